// BuildingLoader.h -- the reference's CSV mesh loader (S/BuildingLoader.h, S/BuildingLoader.cpp:36-290) on top of the C ABI:
// the vertex and face CSVs are parsed on the host as the reference parses them, and the mesh is voxelized on the GPU by
// rto_voxelize_mesh (include/rto_hip.h), bit for bit the reference's grid.  The GDB loaders the reference
// declares next to it were never defined there and are not here either.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "OctreeVoxel.h"

// The two CSVs resolved for rto_voxelize_mesh.  xyz: every vertex row that parsed (x = easting, y = northing, z = elevation),
// all of them count for the grid's bounds; tris: row indices of the faces whose three vertices were found, each (mesh, vertex
// number) naming the LAST row with that key.  Rows: header skipped, blank lines skipped, tokens split on ',' and trimmed of
// " \t\n\r", vertex rows need 8 tokens and face rows 4, a row whose stoi / stod throws is skipped.
struct CSVMesh {
    std::vector<double> xyz;
    std::vector<int32_t> tris;
    int64_t vertexRows = 0;          // rows that parsed
    int64_t faceRows = 0;
};
CSVMesh loadCSVMesh(const std::string& vertsFilename, const std::string& facesFilename);

// S/BuildingLoader.cpp:153-290: the grid from the mesh's bounds and voxelSize, not recentred (main.cpp recentres it afterwards:
// VoxelGrid + recenterFilledVoxels, or RayTracerBVH::loadMesh with recenterPasses).  No vertex row or no face row: an empty grid,
// as the reference returns.  Voxelized on GPU 0; on a failure the grid is empty and the reason goes to std::cerr.
VoxelGrid loadCSVDataIntoVoxelGrid(const std::string& vertsFilename, const std::string& facesFilename, float voxelSize = 5.0f);
