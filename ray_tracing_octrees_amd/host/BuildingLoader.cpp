// BuildingLoader.cpp -- see BuildingLoader.h.
#include "BuildingLoader.h"

#include <fstream>
#include <iostream>
#include <sstream>
#include <unordered_map>

#include "RayTracerBVH.h"

namespace {

std::string trimmed(const std::string& s) {
    const char* ws = " \t\n\r";
    const size_t a = s.find_first_not_of(ws);
    if (a == std::string::npos) return std::string();
    return s.substr(a, s.find_last_not_of(ws) - a + 1);
}

// Calls row(tokens) for every data line of the file with at least minTokens tokens; false when the file cannot be opened.
template <class F> bool forEachRow(const std::string& filename, size_t minTokens, F&& row) {
    std::ifstream in(filename);
    if (!in) return false;
    std::string line, tok;
    std::getline(in, line);                         // header
    std::vector<std::string> t;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        t.clear();
        std::istringstream ss(line);
        while (std::getline(ss, tok, ',')) t.push_back(trimmed(tok));
        if (t.size() < minTokens) continue;
        try {
            row(t);
        } catch (const std::exception&) {
            std::cerr << "[BuildingLoader] skipped unparsable row: " << line << std::endl;
        }
    }
    return true;
}

}  // namespace

CSVMesh loadCSVMesh(const std::string& vertsFilename, const std::string& facesFilename) {
    CSVMesh m;
    std::unordered_map<int64_t, int32_t> rowOf;     // (mesh, vertex number) -> last row
    auto key = [](int mesh, int v) { return (int64_t)mesh * 4294967296ll + (int64_t)(uint32_t)v; };
    if (!forEachRow(vertsFilename, 8, [&](const std::vector<std::string>& t) {
            const int mesh = std::stoi(t[0]), vnum = std::stoi(t[1]);
            double v[6];
            for (int i = 0; i < 6; i++) v[i] = std::stod(t[2 + i]);   // latitude, longitude, elevMin parse too (or the row is skipped)
            rowOf[key(mesh, vnum)] = (int32_t)m.vertexRows;
            m.xyz.insert(m.xyz.end(), { v[0], v[1], v[2] });
            m.vertexRows++;
        }))
        std::cerr << "[BuildingLoader] cannot open vertex file " << vertsFilename << std::endl;
    if (!forEachRow(facesFilename, 4, [&](const std::vector<std::string>& t) {
            const int mesh = std::stoi(t[0]);
            const int v[3] = { std::stoi(t[1]), std::stoi(t[2]), std::stoi(t[3]) };
            m.faceRows++;
            int32_t r[3];
            for (int k = 0; k < 3; k++) {
                const auto it = rowOf.find(key(mesh, v[k]));
                if (it == rowOf.end()) return;      // a vertex is missing: the face is skipped
                r[k] = it->second;
            }
            m.tris.insert(m.tris.end(), { r[0], r[1], r[2] });
        }))
        std::cerr << "[BuildingLoader] cannot open face file " << facesFilename << std::endl;
    return m;
}

VoxelGrid loadCSVDataIntoVoxelGrid(const std::string& vertsFilename, const std::string& facesFilename, float voxelSize) {
    const CSVMesh m = loadCSVMesh(vertsFilename, facesFilename);
    if (m.vertexRows == 0 || m.faceRows == 0) return VoxelGrid();
    std::vector<int32_t> tris = m.tris;
    // Face rows exist but none resolved: the reference still returns its (all EMPTY) grid.  One face on row 0 three times is
    // degenerate (denom 0), so it fills nothing and the AUTO grid is still made.
    if (tris.empty()) tris.assign(3, 0);
    RayTracerBVH rt;
    if (!rt.loadMesh(m.xyz.data(), m.vertexRows, tris.data(), (int64_t)(tris.size() / 3), voxelSize, 0, false)) {
        std::cerr << "[BuildingLoader] voxelization failed: " << rt.lastError() << std::endl;
        return VoxelGrid();
    }
    return rt.grid();
}
