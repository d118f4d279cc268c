/*
 * rto_hip.h -- C ABI of librto_hip.so: the MI355X (gfx950) replacement for the
 * device side of the reference's RayTracerBVH.
 *
 * The reference (abodthedude25/Ray_Tracing_Octrees, 453-skeleton/ = S/) has no
 * FFI: its "device boundary" is the OpenGL driver.  Each entry point below
 * replaces the GL calls named next to it; the C++ class in
 * ray_tracing_octrees_amd/host/RayTracerBVH.h keeps the reference's own
 * signatures (S/RayTracerBVH.h:28-80) on top of this ABI, and INTEGRATION.md
 * shows the binding a maintainer of the reference would add.
 *
 * Plain C types only: pointers, sizes, floats.  Matrices are column-major
 * float[16] exactly as glm::mat4 lays them out (&view[0][0],
 * S/RayTracerBVH.cpp:671).  All functions return RTO_OK (0) or a negative
 * RTO_E* code; rto_last_error() gives the message.  A context is bound to one
 * GPU; calls on one context must be serialised by the caller (the reference is
 * single-threaded, S/main.cpp), different contexts may be driven concurrently.
 */
#ifndef RTO_HIP_H
#define RTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTO_OK            0
#define RTO_E_INVALID    -1   /* bad argument                                  */
#define RTO_E_NO_OCTREE  -2   /* render before rto_upload_octree               */
#define RTO_E_HIP        -3   /* HIP runtime error (message has the hipError)  */
#define RTO_E_NO_DEVICE  -4   /* no usable gfx950 device / ordinal out of range */
#define RTO_E_UNSUPPORTED -5  /* e.g. packed kernel requested for a non-canonical array */
#define RTO_E_TIMEOUT    -6   /* rto_comm_flush_timeout: the collective did not complete; the communicator was aborted and is dead */
#define RTO_E_INTERNAL   -7   /* a bounded device loop hit its cap (rto_label_components): a defect, never an input error */

/* == struct GPUNodes, S/RayTracerBVH.h:21-26 / GLSL OctreeNodeGPUStruct S/RayTracerBVH.cpp:195-204 */
typedef struct rto_node {
    int32_t x, y, z, size;
    int32_t isLeaf, isSolid, isUniform;
    int32_t child[8];              /* -1 = none */
} rto_node;                        /* 60 bytes, stride 60 */

/* The uniforms of S/RayTracerBVH.cpp:652-680 that the shader actually reads
 * (numNodes and invVP are set by the reference but unused by the GLSL). */
typedef struct rto_frame {
    float   view[16];              /* camera.getView(), column-major           :668,:671 */
    float   cam_pos[3];            /* camera.getPos()                          :673-674 */
    float   aspect;                /*                                          :676     */
    float   fov_deg;               /* degrees                                  :677     */
    int32_t width, height;         /*                                          :679-680 */
} rto_frame;

/* Screen-space partition for multi-GPU rendering (no reference counterpart,
 * SURVEY.md section 8e): the image is cut into bands of band_rows rows; band b
 * belongs to part (b % num_parts).  A part's bands are stored back to back in
 * its compact buffer.  {1, 0, any} = the whole frame. */
typedef struct rto_partition {
    int32_t num_parts;
    int32_t part;
    int32_t band_rows;             /* multiple of 8 */
} rto_partition;

/* Which traversal kernel runs. AUTO = PACKED when the uploaded array is a
 * canonical BFS octree (what setOctree produces), else GENERIC. */
#define RTO_KERNEL_AUTO    0
#define RTO_KERNEL_GENERIC 1       /* 60-byte nodes, explicit child indices, per-thread stack[141] */
#define RTO_KERNEL_PACKED  2       /* 8-byte child descriptors, LDS level stack, branch-free O(1)-ascent loop with the pop
                                    * count rebuilt once per ray after the loop (k_trace_lean) */
#define RTO_KERNEL_PACKED_V1 3     /* first form of the packed kernel (level-by-level ascent); kept for A/B runs */
#define RTO_KERNEL_PACKED_PERSISTENT 4  /* the default kernel as persistent threads: a machine-filling grid whose waves
                                         * take launch slots from a global counter; kept for A/B runs */
#define RTO_KERNEL_PACKED_V3 5     /* round-1 default (k_trace_packed3: pops counted inside the loop); kept for A/B runs */

typedef struct rto_stats {         /* per-frame counters, same meaning as the oracle's */
    uint64_t rays, pops, hits, capped;
} rto_stats;

typedef struct rto_octree_info {
    int64_t num_nodes;             /* as uploaded                                         */
    int64_t num_internal;          /* nodes that push children                            */
    int32_t root_size;
    int32_t depth;                 /* log2(root_size)                                     */
    int32_t canonical;             /* 1 if the packed kernel can be used                  */
    int32_t culling_active;        /* 1 after rto_update_frustum(enable=1)                */
    int64_t visible_nodes;         /* count kept by the last frustum update (== num_nodes if none) */
} rto_octree_info;

typedef struct rto_context rto_context;

/* ---- lifetime -------------------------------------------------------------
 * replaces: GL context + RayTracerBVH::ensureComputeInitialized (S/RayTracerBVH.cpp:508-612). */
int  rto_create(int device_ordinal, rto_context** out);
void rto_destroy(rto_context* ctx);
const char* rto_last_error(const rto_context* ctx);     /* ctx may be NULL: error of the last failed rto_create */
int  rto_device_name(const rto_context* ctx, char* buf, size_t buflen);

/* ---- octree upload --------------------------------------------------------
 * replaces: glBufferData(GL_SHADER_STORAGE_BUFFER, numNodes*sizeof(GPUNodes), ...) in
 * RayTracerBVH::setOctree (S/RayTracerBVH.cpp:495-504).  The array is copied; the
 * library additionally repacks canonical arrays into child descriptors.  Refused:
 * a child index outside the array (RTO_E_INVALID); a cycle, a node larger than
 * 2^20 voxels, or a walk from node 0 that could hold more than 7*20+1 stack
 * entries (RTO_E_UNSUPPORTED).  Canonical octrees of depth <= 20 always pass. */
int  rto_upload_octree(rto_context* ctx, const rto_node* nodes, int64_t num_nodes,
                       const float grid_min[3], float voxel_size);
/* N4 -- replaces createOctreeFromVoxelGrid + the BFS of setOctree + the upload (S/OctreeVoxel.cpp:704-778,
 * S/RayTracerBVH.cpp:443-504) in one call: the voxel grid (VoxelGrid.data layout: 1 byte per voxel, 0 EMPTY /
 * 1 FILLED, x fastest) is copied to the GPU and the flat GPUNodes array + child descriptors are built there
 * (occupancy pyramid, level-order emission).  The resident array is byte-identical to what the reference's two
 * functions produce; rto_download_nodes returns it. */
int  rto_build_octree(rto_context* ctx, const uint8_t* voxels, int dim_x, int dim_y, int dim_z,
                      const float grid_min[3], float voxel_size);
int  rto_download_nodes(rto_context* ctx, rto_node* out, int64_t capacity, int64_t* count);   /* out may be NULL */
/* Developer aid: rto_build_octree has two forms that produce the same arrays -- four launches for any depth (pyramid
 * levels kept in Morton order, every tree level ranked and emitted at once; grids up to 1024^3) and a level-by-level
 * form (~5 launches per level; any size).  level_by_level != 0 forces the second, 0 restores the automatic choice. */
int  rto_debug_set_build_path(rto_context* ctx, int level_by_level);
/* Device time of the last rto_build_octree: kernels (pyramid + emission) and the host-to-device voxel copy. */
int  rto_last_build_ms(const rto_context* ctx, float* kernels_ms, float* upload_ms);
int  rto_octree_info_get(const rto_context* ctx, rto_octree_info* out);
int  rto_set_kernel(rto_context* ctx, int kernel /* RTO_KERNEL_* */);
/* Launch order of the 8x8-pixel tiles in the packed kernel (a scheduling hint; pixels never depend on it).
 * Only the tiles of the root box's screen rectangle get a wave; the frame ends when its deepest rays end, so the
 * waves that will run longest should start first.
 * CENTRE_OUT: outwards from the projection of the solid geometry's centre.  TEMPORAL (default): by the per-tile
 * trip counts earlier frames of the same size recorded (CENTRE_OUT until one exists); the table is rebuilt by one
 * small kernel in front of a frame whenever the rectangle's tile box changed its size, and otherwise after refresh_period
 * frames (default 8; 0 keeps the current period) -- an interval that doubles, up to 8 x refresh_period, for as long as the
 * box keeps its size (a camera that stands still or pans). */
#define RTO_ORDER_CENTRE_OUT 0
#define RTO_ORDER_TEMPORAL   1
int  rto_set_launch_order(rto_context* ctx, int policy, int refresh_period);
/* The launch-order tables belong to the launch stream (hipStream_t as void*).  A context keeps them for the 16 most
 * recently used streams; call this before destroying a stream so that a later stream that happens to get the same
 * handle does not inherit its table (harmless to pixels, a stale schedule).  Synchronises the device. */
int  rto_forget_stream(rto_context* ctx, void* hip_stream);

/* ---- frustum culling ------------------------------------------------------
 * replaces: the CPU loop + compaction + SSBO re-upload of
 * renderSceneComputeWithCulling(updateFrustum=true) (S/RayTracerBVH.cpp:725-813).
 * The test runs on the GPU over the resident array; rendering afterwards behaves as
 * if the compacted array had been uploaded.  enable=0 restores the full array.
 * For canonical BFS octrees (what setOctree / rto_build_octree produce) the update is ONE kernel on rto_stream(ctx) and reads
 * nothing back: the visibility flags, the descriptors' visibility bits, the number of surviving nodes and the node traversals
 * start at (the root; the first visible node when the root itself was culled, S/RT:765-812) stay on the device, where the
 * traversal kernels read them; rto_octree_info_get / rto_download_visible_nodes fetch the count when asked (they wait for the
 * device).  The compacted array itself is made when somebody needs it (rto_download_visible_nodes, the generic kernel).
 * Ordering: frames on the context's own stream are ordered around the update by the stream; if frames were launched on other
 * streams since the last update (or ever captured on one), the device is waited for first.  Other arrays: per-node test,
 * one read-back (synchronous).  Before any of that the host asks whether the planes can cull a node at all (see
 * rto_debug_set_frustum_shortcut): when provably not, nothing is launched. */
int  rto_update_frustum(rto_context* ctx, const float view[16], float fov_deg, float aspect, int enable);
/* Developer aid: the same update with caller-supplied planes (LEFT, RIGHT, TOP, BOTTOM, NEAR, FAR as nx, ny, nz, d;
 * normalised) and margin instead of the ones S/RT:731-755 derives -- lets a test build situations real cameras cannot,
 * e.g. a culled root with surviving descendants (S/RT:765-812 then starts at whatever lands at compacted index 0). */
int  rto_debug_update_frustum_planes(rto_context* ctx, const float planes[24], float margin);
/* rto_update_frustum first asks, on the host, whether the planes can cull ANY node: every box lies in the root's, so a lower
 * bound of the positive-vertex value over all nodes is one expression per plane; when it exceeds the float evaluation's
 * possible error a thousandfold for all six planes -- with the reference's margin of 150 units: every camera near a scene a
 * few units across -- every node is visible, the device state that says so is written once and further such updates launch
 * NOTHING (identical results, S/RT:743-802's loop passes every node as well).  enabled = 0 forces the kernel (A/B, tests). */
int  rto_debug_set_frustum_shortcut(rto_context* ctx, int enabled);
/* *proven = 1 when the last frustum update was answered by that proof (no kernel), else 0. */
int  rto_debug_last_frustum_update_proven(const rto_context* ctx, int* proven);
/* Copies the compacted array (== m_visibleNodes, S/RayTracerBVH.cpp:775-802) to the host for parity
 * checks.  out may be NULL to query the count only. */
int  rto_download_visible_nodes(rto_context* ctx, rto_node* out, int64_t capacity, int64_t* count);

/* ---- render ---------------------------------------------------------------
 * replaces: glTexImage2D(RGBA32F) + uniforms + glDispatchCompute + glMemoryBarrier
 * (S/RayTracerBVH.cpp:630-688).  Output: RGBA32F, row-major, row 0 = top, alpha 1. */

/* Asynchronous: renders this part's bands into d_out (device pointer,
 * rto_partition_rows()*width*16 bytes) on hip_stream, a hipStream_t passed as void*.
 * As everywhere in HIP, NULL is the default (null) stream; rto_stream() returns the
 * context's own non-blocking stream for callers that want one. */
int  rto_render_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part /* NULL = whole frame */,
                       void* d_out, void* hip_stream);
/* HIP graphs: once a frame of the same width/height/aspect/fov has been rendered on a stream, rto_render_device (and the
 * _shade / _triangles variants) allocate nothing and never synchronise on it, so a sequence of frames may be captured
 * with hipStreamBeginCapture and replayed; a captured launch that WOULD have to allocate or synchronise (first frame of
 * a new size on that stream) fails with RTO_E_UNSUPPORTED instead of invalidating the capture (the runtime needs ~9 us between dependent plain launches but ~1 us between
 * graph nodes: 70 -> 61 us per frame at BASELINE config 2).  Captured launches use a launch-order table of their own (plain
 * launches never read it), and the first frame a capture records on a stream always carries a table-rebuild node, so a replay
 * never depends on what plain launches, other graphs or its own last frame left behind.  Replay a graph on the stream it was
 * captured on: the tables belong to that stream.  rto_update_frustum (canonical octrees, after one plain call) and
 * rto_render_resident can be captured on rto_stream(ctx) the same way: the update reads nothing back. */
/* Synchronous convenience: whole frame into host memory (the one API addition the
 * reference lacks: its texture is never read back). */
int  rto_render_host(rto_context* ctx, const rto_frame* frame, float* host_rgba);
/* The reference renders into a GL texture that stays on the GPU (S/RayTracerBVH.cpp:630-646, 684-688) and never reads
 * it back.  Same here: rto_render_resident renders the whole frame into the context's own device framebuffer
 * (asynchronous, on rto_stream(ctx)); mode RTO_RESIDENT_OCTREE = the octree path, RTO_RESIDENT_TRIANGLES /
 * RTO_RESIDENT_TRIANGLES_SHADOW = the leaf-triangle path of config 5.  rto_resident_frame returns the device pointer
 * (RGBA32F, width*height*16 bytes; valid until a render of another size or rto_destroy) for display interop or further
 * device work; rto_download_resident copies it to the host (synchronises). */
#define RTO_RESIDENT_OCTREE 0
#define RTO_RESIDENT_TRIANGLES 1
#define RTO_RESIDENT_TRIANGLES_SHADOW 2
int  rto_render_resident(rto_context* ctx, const rto_frame* frame, int mode);
int  rto_resident_frame(rto_context* ctx, void** d_rgba, int* width, int* height);
int  rto_download_resident(rto_context* ctx, float* host_rgba);
/* Number of rows part `part` owns. */
int  rto_partition_rows(const rto_frame* frame, const rto_partition* part);
/* Reassembles num_parts compact buffers laid end to end (as a gather delivers them;
 * every part padded to rto_partition_rows(part 0) rows) into a row-major frame. */
int  rto_assemble_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part,
                         const void* d_gathered, void* d_frame, void* hip_stream);
/* The same pair with a 4-byte payload per pixel, for the xGMI gather (no reference counterpart: the reference is
 * single-GPU).  Every pixel of S/RayTracerBVH.cpp:331-336 / :363 is a function of ONE float -- the Lambert term
 * max(dot(n, -L), 0) of the hit, or "no hit" -- so a part ships that float (-1.0f = no hit: rows*width*4 bytes
 * instead of *16) and the gathering GPU finishes `vec3(1,.8,.6) * term + .1` while it re-interleaves.  Same float
 * operations in the same order: the assembled frame is bit-identical to rto_render_device's. */
int  rto_render_shade_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part /* NULL = whole frame */,
                             void* d_shade, void* hip_stream);
int  rto_assemble_shade_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part,
                               const void* d_gathered_shade, void* d_frame, void* hip_stream);
/* Fewer, larger collectives: when every rank ships `batch` consecutive frames of its part in ONE gather
 * ([rank][batch][part-0 rows][width], either payload), this rebuilds frame `index` of the batch. */
int  rto_assemble_batch_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part, const void* d_gathered,
                               int batch, int index, int shade_payload, void* d_frame, void* hip_stream);
/* Several frames at once: this part (NULL: the whole frame) of frames[0..n-1] (any cameras, same width/height) into
 * d_out + i*frame_stride_bytes, either payload, asynchronously on hip_stream, up to 8 frames per kernel launch.  One frame's
 * kernel cannot be shorter than the ~36 us its deepest tile needs for its chain of dependent node visits, with most of the
 * GPU idle meanwhile; frames rendered together fill it (config 2: 46 -> 36 us per frame; a rank of an 8-GPU split: 36 -> 6 us
 * per part).  Pixels are those of n rto_render_device calls.  This is the throughput form: a caller that must show frame i
 * before it knows frame i+1's camera keeps using rto_render_device.
 * rto_assemble_batch_all_device: all `batch` frames of a gather into d_frames + i*frame_stride_bytes. */
int  rto_render_batch_device(rto_context* ctx, const rto_frame* frames, int n, const rto_partition* part, int shade_payload,
                             void* d_out, size_t frame_stride_bytes, void* hip_stream);
int  rto_assemble_batch_all_device(rto_context* ctx, const rto_frame* frames, int batch, const rto_partition* part,
                                   const void* d_gathered, int shade_payload, void* d_frames, size_t frame_stride_bytes, void* hip_stream);

/* ---- multi-GPU: screen split + ONE gather per batch, below the C boundary ---------------------------------
 * No reference counterpart (the reference is single-GPU).  A communicator binds one context
 * (= one GPU, holding the whole octree) to a rank of a world of GPUs of one node.  rto_comm_submit renders this rank's
 * bands (band b of band_rows rows belongs to rank b % world; from 4 ranks on rank 0 only gathers and assembles and band b
 * belongs to rank 1 + b % (world - 1)) of n consecutive frames as the 4-byte payload of
 * rto_render_shade_device, ships them to rank 0 with ONE grouped ncclSend/ncclRecv (RCCL over xGMI: a direct gather into
 * the root, never a ring) and, on rank 0, re-interleaves and finishes the colours into d_frames + i*frame_stride_bytes
 * (RGBA32F, bit-identical to rto_render_device).  Asynchronous and pipelined: the call returns when the work is
 * enqueued on the communicator's own two HIP streams, the gather of batch k overlaps the render of batch k+1 (two
 * sets of buffers alternate); d_frames must stay valid until rto_comm_flush (or a wait on rto_comm_stream) returns.
 * Every rank makes the same sequence of calls.  mode: RTO_RESIDENT_OCTREE / _TRIANGLES / _TRIANGLES_SHADOW.
 *
 * One process per GPU: rank 0 calls rto_comm_unique_id, hands the RTO_COMM_ID_BYTES bytes to the other ranks by any
 * means (MPI, a TCP store, a file), every rank calls rto_comm_create.  One process, several GPUs (what
 * RayTracerBVH::setDevices uses): rto_comm_create_all over n contexts on n different devices, then
 * rto_comm_submit_all issues every rank's part of a batch from the calling thread.  librccl is loaded on first use. */
typedef struct rto_comm rto_comm;
#define RTO_COMM_ID_BYTES 128
int  rto_comm_unique_id(void* id /* RTO_COMM_ID_BYTES */);
int  rto_comm_create(rto_context* ctx, int world, int rank, const void* id, int band_rows, rto_comm** out);
int  rto_comm_create_all(rto_context* const* ctxs, int n, int band_rows, rto_comm** out /* n handles */);
void rto_comm_destroy(rto_comm* comm);
const char* rto_comm_last_error(const rto_comm* comm);
int  rto_comm_submit(rto_comm* comm, const rto_frame* frames, int n, int mode, void* d_frames /* rank 0 */, size_t frame_stride_bytes);
int  rto_comm_submit_all(rto_comm* const* comms, int n_comms, const rto_frame* frames, int n, int mode, void* d_frames, size_t frame_stride_bytes);
/* single-process group: one frame through all ranks into rank 0's resident framebuffer (cf. rto_render_resident);
 * asynchronous, rto_download_resident / rto_resident_frame of rank 0's context give the assembled frame */
int  rto_comm_render_resident_all(rto_comm* const* comms, int n_comms, const rto_frame* frame, int mode);
int  rto_comm_flush(rto_comm* comm);              /* waits until every submitted batch is complete on this rank; reports an asynchronous
                                                     RCCL error of the communicator (ncclCommGetAsyncError) as RTO_E_HIP and marks it dead */
/* The same with a limit: polls the communicator's two streams (and its asynchronous error state) for at most timeout_ms.  On expiry
 * -- a peer died before its ncclSend, a link is down: without a limit rank 0 would sit in hipStreamSynchronize for ever -- or on an
 * asynchronous RCCL error the communicator is aborted (ncclCommAbort), marked DEAD and RTO_E_TIMEOUT / RTO_E_HIP is returned.  A dead
 * communicator refuses every further submit / flush (RTO_E_INVALID, "communicator is dead"); rto_comm_destroy still returns (it does
 * not wait for streams of a dead communicator's aborted collectives beyond their completion by the abort).  timeout_ms <= 0: no limit
 * (as rto_comm_flush). */
int  rto_comm_flush_timeout(rto_comm* comm, int timeout_ms);
/* 1 once the communicator has been aborted (timeout or asynchronous error), else 0.  The communicators of ONE
 * rto_comm_create_all group die together: every batch queues a Send / Recv on each of them, so an abort of one member aborts
 * (and marks dead) all of them, and rto_comm_submit_all checks every member before any of them starts the batch.
 * rto_comm_destroy never waits on a collective that cannot finish: it polls the streams (10 s) and aborts a live communicator
 * whose streams stay busy (a peer process that died) before it releases anything. */
int  rto_comm_is_dead(const rto_comm* comm);
/* ncclCommCount of the live communicator: the ranks RCCL itself says take part (what an N-GPU bench line reports as ranks_seen). */
int  rto_comm_ranks_seen(const rto_comm* comm, int* ranks);
/* Test hook: marks the communicator as timed out exactly as rto_comm_flush_timeout does on expiry (ncclCommAbort, dead). */
int  rto_comm_debug_abort(rto_comm* comm);
/* Developer aid: a ONE-rank communicator renders, ships and assembles as rank as_rank of as_world GPUs (every per-rank cost
 * of an N-GPU split except the other GPUs' traffic); the assembled frames hold that rank's bands only.  as_world = 0: off. */
int  rto_comm_debug_rehearse(rto_comm* comm, int as_world, int as_rank);
/* Developer aid: floats this rank shipped for the batch submitted last -- only the columns of the geometry's screen rectangle
 * travel, rank 0 paints the background itself -- and what whole rows would have been. */
int  rto_comm_debug_set_rehearsal_clear(rto_comm* comm, int enabled);   /* rehearsals: per-batch clear of the absent ranks' rows (default on; timing runs switch it off) */
int  rto_comm_debug_last_payload(const rto_comm* comm, int64_t* packed_floats, int64_t* full_floats);
/* Bench aid: with timing on, every batch records four timed events; after its flush rto_comm_debug_last_timing gives the GPU
 * milliseconds of the batch submitted last: ms[0] this rank's render (+ pack), ms[1] its grouped send / recv (+ rank 0's assembly). */
int  rto_comm_debug_set_timing(rto_comm* comm, int enabled);
int  rto_comm_debug_last_timing(rto_comm* comm, float ms[2]);
void* rto_comm_stream(rto_comm* comm);            /* hipStream_t the gathers and (rank 0) the assembled frames are ordered on */

/* ---- multi-GPU: the split plan (pure host arithmetic, no GPU needed) -----------------------------------------
 * Everything the ranks of a screen split must agree on BEFORE they post sends and receives -- who renders, which part a
 * rank owns, the rows every part's buffer is padded to, the column window of each frame of the batch that travels (only
 * the columns of the geometry's screen rectangle do), the offsets inside a packed part and the float count per rank --
 * is derived by ONE function from the frames and the scene's bounds.  rto_comm_submit calls it on every rank; tests call
 * the same function from N processes and compare the plans byte for byte (tests/_tilesplit_worker.py), so a mismatch
 * cannot first appear as a hang inside RCCL.  No reference counterpart (the reference is single-GPU). */
typedef struct rto_scene_bounds {
    float   grid_min[3];
    float   voxel_size;
    int32_t root_size;             /* octree root edge in voxels (power of two)                      */
    int32_t solid_lo[3], solid_hi[3];  /* bounding box of the solid leaves, voxel units; lo > hi: nothing solid */
} rto_scene_bounds;
int  rto_scene_bounds_get(const rto_context* ctx, rto_scene_bounds* out);
/* the same from a GPUNodes array on the host (what rto_upload_octree derives) */
int  rto_scene_bounds_of_nodes(const rto_node* nodes, int64_t num_nodes, const float grid_min[3], float voxel_size, rto_scene_bounds* out);

#define RTO_SPLIT_MAX_FRAMES 32    /* frames of one batch whose windows the plan can hold; larger batches ship whole rows */
typedef struct rto_split_plan {
    int32_t world, band_rows, width, height, n_frames;
    int32_t render_parts;          /* parts a frame is cut into: world, or world - 1 when rank 0 only gathers (world >= 4) */
    int32_t first_render_rank;     /* 0, or 1 when rank 0 only gathers and assembles                 */
    int32_t rows_part0;            /* rows of part 0 = rows every part's buffer is padded to          */
    int32_t cropped;               /* 1: only the window columns of each frame travel                 */
    int32_t win_x0[RTO_SPLIT_MAX_FRAMES], win_w[RTO_SPLIT_MAX_FRAMES];   /* window of frame i: columns [x0, x0 + w) */
    int64_t win_off[RTO_SPLIT_MAX_FRAMES];   /* float offset of frame i inside a rank's packed part (rows_part0 x win_w each) */
    int64_t frame_floats;          /* rows_part0 * width: one frame of a part, unpacked               */
    int64_t full_floats;           /* frame_floats * n_frames                                         */
    int64_t pack_floats;           /* floats every rendering rank ships == stride between the parts on rank 0 */
} rto_split_plan;
int  rto_split_plan_make(const rto_scene_bounds* scene, const rto_frame* frames, int n, int world, int band_rows, rto_split_plan* out);
int  rto_split_part_of_rank(const rto_split_plan* plan, int rank);      /* part that rank renders, -1: it renders nothing */
int  rto_split_rows_of_part(const rto_split_plan* plan, int part);      /* rows part owns (<= rows_part0)                */
/* Where row `row` of an assembled frame comes from: *part and the row inside that part's compact buffer. */
int  rto_split_row_source(const rto_split_plan* plan, int row, int* part, int* local_row);

/* ---- N2: leaf triangles + shadow ray (BASELINE config 5) -------------------------
 * No upstream counterpart: the reference has no ray/triangle code (its MC triangles are rasterised).  The
 * triangles are those MarchingCubesRenderer emits per leaf (localMC, S/OctreeVoxel.cpp:780-879;
 * host/OctreeVoxel.h buildLeafTriangles): 12 floats each (v0, v1, v2, face normal), ordered by node;
 * tri_offset[i]..tri_offset[i+1] (numNodes+1 entries) is node i's range.  Rendering follows the reference's
 * traversal order and 512-pop cap; a leaf is hit when one of its triangles is (Moeller-Trumbore, nearest
 * t > 0 in the leaf); shading = the reference's Lambert term on the ray-facing face normal; shadow != 0 adds one
 * ray towards the light (any hit => ambient only).  stats may be NULL (pops counts both traversals).
 * Frustum state: the triangle render walks the whole array's triangle records, which a compacted array does not have.  While
 * an rto_update_frustum(enable=1) is in force every rto_render_triangles_* entry, and rto_render_resident in its two triangle
 * modes, fails with
 * RTO_E_UNSUPPORTED ("render_triangles: not available while frustum culling is active")
 * and changes nothing; after rto_update_frustum(enable=0) it renders again, bit for bit.  The triangle queries and the lit
 * triangle render below ignore the update instead. */
int  rto_upload_leaf_triangles(rto_context* ctx, const float* tris, int64_t num_tris, const int32_t* tri_offset);
/* The same buffer built in HBM (replaces the CPU loop MarchingCubesRenderer::render -> localMC per leaf,
 * S/Renderer.cpp:14-36, S/OctreeVoxel.cpp:780-879): identical triangles in identical order, for the resident octree.
 * voxels: dimX*dimY*dimZ bytes (x fastest, 0 EMPTY / 1 FILLED) of the grid the octree was made from; NULL (dims
 * ignored) reuses the voxels rto_build_octree kept in HBM.  rto_last_build_ms() then reports this build.
 * rto_download_leaf_triangles copies the result out for parity checks (tris / tri_offset may be NULL). */
int  rto_build_leaf_triangles(rto_context* ctx, const uint8_t* voxels, int dimX, int dimY, int dimZ);
int  rto_download_leaf_triangles(rto_context* ctx, float* tris, int64_t tri_capacity, int32_t* tri_offset /* numNodes+1 */,
                                 int64_t* num_tris);
int  rto_render_triangles_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part, int shadow,
                                 void* d_out, void* hip_stream);
/* Several frames per kernel launch, as rto_render_batch_device: this part (NULL: whole frames) of frames[0..n-1] into
 * d_out + i*frame_stride_bytes, RGBA32F or (shade_payload) the 4-byte Lambert term.  A part's kernel lasts as long as its
 * deepest tile (0.24 ms at config 5 whatever its share of the pixels); parts launched together fill the GPU. */
int  rto_render_triangles_batch_device(rto_context* ctx, const rto_frame* frames, int n, const rto_partition* part, int shadow, int shade_payload,
                                       void* d_out, size_t frame_stride_bytes, void* hip_stream);
int  rto_render_triangles_host(rto_context* ctx, const rto_frame* frame, int shadow, float* host_rgba, rto_stats* stats);
/* 4-byte payload variant (see rto_render_shade_device); reassemble with rto_assemble_shade_device. */
int  rto_render_triangles_shade_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part, int shadow,
                                       void* d_shade, void* hip_stream);

/* ---- N1: octreeRaySkip --------------------------------------------------------
 * replaces: the CPU recursion octreeRaySkip(root, ro, rd, tMin, tMax, grid, &visibility)
 * (S/VolumeRaycastRenderer.cpp:50-155; called for a 7x7 probe grid per frame at :1602-1647).
 * n rays share the origin ro; rd holds n directions (x,y,z).  out_t[i] = entry distance of the first solid
 * leaf in the reference's child order, or 1e30.  use_visibility != 0 applies the flags of the last
 * rto_update_frustum the way the reference applies its visibility map (:64-67).  Synchronous, host buffers. */
int  rto_octree_ray_skip(rto_context* ctx, const float ro[3], const float* rd, int64_t n, float t_min, float t_max,
                         int use_visibility, float* out_t);

/* The reference's CLOSEST-hit traversal -- the earlier compute shader it keeps block-commented in the same file
 * (453-skeleton/RayTracerBVH.cpp:46-166; traversal :63-138): the rays, slab test, LIFO order and shading of rto_render_device, but no
 * break on the first accepted leaf and no 512-pop cap: every node whose tNear lies below the best hit so far is visited, the solid
 * leaf with the smallest tHit = max(0, tNear) wins, a later leaf replacing it only when strictly nearer.  Dead code upstream
 * (replaced by the "workload limiting" shader rto_render_device implements), the only traversal rule of the reference this library
 * could not render until round 4.  Pixels are bit-identical to that shader's text compiled under the reference's glm
 * (oracle/glsl_driver.cpp, tests/golden/glsl_images_small.npz).  RGBA32F, row 0 = top, asynchronous on hip_stream; part as in
 * rto_render_device; a frustum update in force is honoured the way the reference's culled render is (compacted array).  Three
 * kernels, one frame: canonical trees walk the descriptor tree near children first (k_closest_near_first: the winner of the
 * exhaustive walk is the leaf of least tHit among those whose ancestors all pass their slab tests, ties to the leaf popped
 * first, whatever the order of the walk); the counters come from the same pops made in the reference's order
 * (k_closest_lean); arbitrary arrays, culled frames and RTO_KERNEL_GENERIC go node by node over the 60-byte array
 * (k_trace_closest).  _host: synchronous; stats (may be NULL): rays, popped nodes (uncapped), hit pixels. */
int  rto_render_closest_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part /* NULL = whole frame */, void* d_rgba, void* hip_stream);
int  rto_render_closest_host(rto_context* ctx, const rto_frame* frame, float* host_rgba, rto_stats* stats /* may be NULL */);

/* The same search as a RENDER MODE (octreeRaySkip "as a second kernel mode = nearest hit"): for every
 * pixel, the ray of generateRay (S/RayTracerBVH.cpp:338-355, origin = cam_pos) goes through
 * octreeRaySkip(root, ro, rd, 0, 1e30, grid, visibility) (S/VolumeRaycastRenderer.cpp:50-155).  d_dist (width*height floats,
 * row 0 = top, may be NULL): the distance it returns, 1e30 = nothing -- bit-identical to the reference's compiled function on
 * those rays (tests/golden/ref_ray_skip.npz "pixels").  d_rgba (RGBA32F, may be NULL): the reference's shade
 * (S/RayTracerBVH.cpp:283-285, 331-336: box-centre pseudo-normal, Lambert + 0.1) of the leaf that distance belongs to, at
 * tHit = that distance; background (0,0,0,1).  Asynchronous on hip_stream, outputs stay on the device; part as in
 * rto_render_device.  Canonical BFS octrees only.  _host: synchronous convenience (either pointer may be NULL). */
int  rto_render_skip_device(rto_context* ctx, const rto_frame* frame, const rto_partition* part /* NULL = whole frame */, int use_visibility,
                            void* d_rgba, void* d_dist, void* hip_stream);
int  rto_render_skip_host(rto_context* ctx, const rto_frame* frame, int use_visibility, float* host_rgba, float* host_dist);
/* octreeRaySkip's CONSUMER in drawRaycast (S/VolumeRaycastRenderer.cpp:1602-1663) in one launch, nothing copied: the 7x7 probe
 * directions through inverse(perspective(45 deg, aspect, 0.1, 5000)) and inverse(view), the 49 traversals, the value std::sort
 * would leave at index int(n * 0.15f) among the valid distances (0 < t < 1e30) x 0.75, and the temporal blend
 * *d_skip = *d_skip * 0.4f + that * 0.6f (`static float lastSkipDistance` of :1658 = the float the caller keeps on the device:
 * set it to 0 before the first frame).  Asynchronous on hip_stream.  _host: the same with a host float (synchronous); probe_t
 * (may be NULL) receives the 49 distances. */
int  rto_probe_skip_device(rto_context* ctx, const float view[16], const float cam_pos[3], float aspect, int use_visibility,
                           void* d_skip /* one float on the device: in = previous value, out = new */, void* hip_stream);
int  rto_probe_skip_host(rto_context* ctx, const float view[16], const float cam_pos[3], float aspect, int use_visibility,
                         float* io_skip, float* probe_t /* 49 floats or NULL */);

/* ---- ray queries ----------------------------------------------------------
 * No reference counterpart as an API: RayTracerBVH.h:14-18 declares struct Ray { origin; direction; } and nothing consumes it;
 * the click handler (main.cpp:646-700) finds the voxel under the cursor by a CPU march over the dense grid
 * (intersectBuildingVoxel, main.cpp:209-).  These trace caller-supplied rays -- or the renders' own pixel rays -- through the
 * whole resident octree and return one record per ray.
 *
 * Acceptance rule.  t_lo = max(t_min, 0).  A solid leaf is accepted when its box and every ancestor's
 * pass the reference's float32 slab test (tNear <= tFar && tFar > 0, S/RT:226-236, glm min/max) with tNear < 1e30 (the
 * renders' closestT, S/RT:242), and tHit = max(t_lo, tNear) satisfies tHit <= tFar and tHit <= t_max; hits at or beyond 1e30
 * (the miss value) are misses.  With (t_min, t_max) = (0, 1e30) this is the renders' rule: FIRST on a frame's pixel rays gives
 * rto_render_device's hits, CLOSEST rto_render_closest_device's, bit for bit.
 * A ray with a NaN in its origin, direction, t_min or t_max, or with t_min > t_max, is a miss; directions with zero components
 * follow the slab formula with its infinite reciprocals.  The whole uploaded octree is seen whatever rto_update_frustum did.
 * Face: the lowest axis whose entry parameter equals tNear, signed by d[axis]; -1 when tHit > tNear (origin inside the box,
 * or t_min clipped the entry). */
typedef struct rto_ray {            /* 32 bytes */
    float ox, oy, oz, t_min;
    float dx, dy, dz, t_max;        /* d need not be normalised; t is in units of d */
} rto_ray;

typedef struct rto_hit {            /* 32 bytes */
    float   t;                      /* tHit of the accepted leaf; 1e30f for a miss */
    int32_t node;                   /* index in the resident array (what rto_download_nodes returns); -1 = miss */
    int32_t face;                   /* entry face 0..5 = 2*axis + (d[axis] < 0); -1 = none (tHit > tNear) or miss */
    int32_t size;                   /* leaf box, voxel units (the node's x, y, z, size); 0 for a miss */
    int32_t x, y, z;
    int32_t reserved;               /* 0 */
} rto_hit;

#define RTO_QUERY_FIRST   0   /* the default render's rule: LIFO pop order, first accepted solid leaf, 512-pop cap */
#define RTO_QUERY_CLOSEST 1   /* rto_render_closest's rule: least tHit, ties to the leaf popped first */
#define RTO_QUERY_ANY     2   /* occlusion: some accepted leaf, or a miss; which leaf is unspecified */

/* Asynchronous on hip_stream; d_rays and d_hits are device pointers, 16-byte aligned.  n == 0: no-op.  RTO_E_INVALID: NULL
 * buffer, unknown mode, n < 0, misaligned buffer; RTO_E_NO_OCTREE: nothing uploaded.  _host: synchronous, host buffers. */
int  rto_query_rays_device(rto_context* ctx, int mode, const rto_ray* d_rays, int64_t n, rto_hit* d_hits, void* hip_stream);
int  rto_query_rays_host(rto_context* ctx, int mode, const rto_ray* rays, int64_t n, rto_hit* hits);
/* rays = the renders' own generateRay for pixel (x, y) of `frame` (row 0 = top), bit-identical to the rays they trace, with
 * (t_min, t_max) = (0, 1e30); d_xy holds n (x, y) int32 pairs.  A pixel outside the frame gets a miss record. */
int  rto_query_pixels_device(rto_context* ctx, int mode, const rto_frame* frame, const int32_t* d_xy, int64_t n,
                             rto_hit* d_hits, void* hip_stream);
int  rto_query_pixels_host(rto_context* ctx, int mode, const rto_frame* frame, const int32_t* xy, int64_t n, rto_hit* hits);

/* ---- triangle queries -----------------------------------------------------
 * The same rays against the resident leaf triangles (rto_build_leaf_triangles / rto_upload_leaf_triangles): the surface
 * rto_render_triangles_* draws.  One rto_tri_hit per ray.  rto_ray, the modes, the pixel rays, the NaN and t_min > t_max misses,
 * the 16-byte alignment, the error codes and the disregard of the frustum state are those of the box queries above.
 *
 * Acceptance rule ("Triangle queries").  A leaf is reachable when its box and every ancestor's pass the
 * float32 slab test with tNear < 1e30 (the triangle render's box rule; boxes see no window).  A triangle of a reachable leaf is
 * accepted when the renders' Moeller-Trumbore test hits it (t > 0) and t_min <= t <= min(t_max, largest float below 1e30).
 *   FIRST    the render's rule: the first leaf in the reference's LIFO pop order that has an accepted triangle, under the
 *            512-pop cap (a capped ray is a miss); in it the least t, ties to the lowest index.  The window decides only which
 *            triangles count, never which nodes are popped.  With (0, 1e30) on a frame's pixel rays: exactly the t and triangle
 *            rto_render_triangles_device shades.
 *   CLOSEST  least t over the accepted triangles of all reachable leaves, ties to the lowest index; no cap.
 *   ANY      a hit exactly when CLOSEST has one; which triangle is unspecified.
 * RTO_E_NO_OCTREE when no leaf triangles are resident: a fresh context, or an rto_upload_octree / rto_build_octree since the last
 * triangle build or upload. */
typedef struct rto_tri_hit {        /* 32 bytes */
    float   t;                      /* Moeller-Trumbore t of the accepted triangle; 1e30f for a miss */
    int32_t tri;                    /* index into the resident triangle buffer (rto_download_leaf_triangles order); -1 = miss */
    int32_t node;                   /* the leaf that owns it (tri_offset[node] <= tri < tri_offset[node+1]); -1 = miss */
    float   u, v;                   /* barycentrics of the hit, as Moeller-Trumbore computes them; 0 for a miss */
    float   nx, ny, nz;             /* the triangle's stored face normal, negated when dot(n, d) > 0 (the renders' turn); 0 for a miss */
} rto_tri_hit;

int  rto_query_triangles_device(rto_context* ctx, int mode, const rto_ray* d_rays, int64_t n, rto_tri_hit* d_hits, void* hip_stream);
int  rto_query_triangles_host(rto_context* ctx, int mode, const rto_ray* rays, int64_t n, rto_tri_hit* hits);
int  rto_query_triangle_pixels_device(rto_context* ctx, int mode, const rto_frame* frame, const int32_t* d_xy, int64_t n,
                                      rto_tri_hit* d_hits, void* hip_stream);
int  rto_query_triangle_pixels_host(rto_context* ctx, int mode, const rto_frame* frame, const int32_t* xy, int64_t n, rto_tri_hit* hits);

/* ---- span queries ---------------------------------------------------------
 * How much solid a ray passes through: the box queries above stop at one leaf, these visit every accepted leaf of the ray and sum.
 * One rto_span per ray.  rto_ray, the pixel rays with window (0, 1e30), the NaN and t_min > t_max misses, the 16-byte alignment of
 * the ray and span buffers, the error codes, the order of the checks, n == 0 and the disregard of the frustum state are those of the
 * box queries.  There is no mode.
 *
 * Rule.  Window: t_lo = max(t_min, 0), t_hi = min(t_max, largest float below 1e30).
 * Acceptance of a solid leaf is the box queries': its box and every ancestor's pass the float32 slab test (tNear <= tFar &&
 * tFar > 0, glm min / max) with tNear < 1e30, and tIn = max(t_lo, tNear) satisfies tIn <= tFar and tIn <= t_hi.
 * For an accepted leaf tOut = min(tFar, t_hi) (glm's min); its contribution is tOut - tIn, one float32 subtraction, >= 0.
 * Visit order (a float sum has one): depth first, the children of a node in slots i ^ flip for i = 0 .. 7 ascending, with
 * flip = (d.x < 0) | (d.y < 0) << 1 | (d.z < 0) << 2 -- a zero or -0.0 component is "not negative".  The order CLOSEST and ANY
 * walk in.  No pop cap.
 * Two identities hold on every ray: (t_enter, node, face) are bit for bit the CLOSEST record of rto_query_rays_* /
 * rto_query_pixels_* for the same ray, and leaves > 0 exactly when ANY hits.  One restriction: the tie between leaves of equal
 * tIn goes by the leaves' positions (at the highest bit in which they differ the greater octant digit x | y << 1 | z << 2 wins),
 * which is the LIFO pop order on every array whose child slots are the octants of the children's boxes -- every octree this
 * library builds, in any numbering.  On an uploaded array with other slots the CLOSEST query breaks such ties by its own pop
 * order, and (node, face) may then differ from it on rays with a tie; t_enter and everything else still agree.
 * RTO_E_UNSUPPORTED: an uploaded non-canonical array whose walk in a ray's octant order (not the slot order rto_upload_octree
 * bounds) could hold more than 141 stack entries -- chains of more than 20 levels; such an array stays resident and every other
 * entry serves it.
 * A miss -- no accepted leaf, NaN input, t_min > t_max, a pixel outside the frame -- is length 0, t_enter 1e30, t_exit 1e30,
 * leaves 0, node -1, face -1.
 * `leaves` counts octree leaves, not walls: a uniform solid region is one large leaf, a wall of depth-max voxels is many.  A run
 * count is deliberately absent: on contiguous leaves tOut of one and tIn of the next are equal as real numbers only, so a merge
 * rule on floats would split runs by one ulp near box edges; `length` has no such discontinuity. */
typedef struct rto_span {           /* 32 bytes */
    float   length;                 /* sum of the contributions, float32, accumulated in visit order from 0.0f; in units of d */
    float   t_enter;                /* least tIn over the accepted leaves; 1e30f for a miss */
    float   t_exit;                 /* greatest tOut over the accepted leaves; 1e30f for a miss */
    int32_t leaves;                 /* number of accepted leaves */
    int32_t node;                   /* CLOSEST's leaf for the same ray: least tIn, ties to the leaf the LIFO order pops first; -1 = miss */
    int32_t face;                   /* its entry face, as rto_hit.face; -1 = none or miss */
    int32_t reserved[2];            /* 0 */
} rto_span;

int  rto_query_spans_device(rto_context* ctx, const rto_ray* d_rays, int64_t n, rto_span* d_spans, void* hip_stream);
int  rto_query_spans_host(rto_context* ctx, const rto_ray* rays, int64_t n, rto_span* spans);
int  rto_query_span_pixels_device(rto_context* ctx, const rto_frame* frame, const int32_t* d_xy, int64_t n, rto_span* d_spans,
                                  void* hip_stream);
int  rto_query_span_pixels_host(rto_context* ctx, const rto_frame* frame, const int32_t* xy, int64_t n, rto_span* spans);

/* ---- voxel edits ----------------------------------------------------------
 * Brushes carve (-> EMPTY = 0) or fill (-> FILLED = 1) the voxel grid rto_build_octree keeps in HBM; the octree is then rebuilt
 * from that grid on the GPU, with no host copy.  Rule, exact in integers at 1/64 voxel:
 *   cq[a] = floor((centre[a] - gridMin[a]) / voxelSize * 64 + 0.5), eq[a] = floor(extent[a] / voxelSize * 64 + 0.5), in double
 *   from the context's float gridMin / voxelSize; D[a] = 64 (2 i[a] + 1) - 2 cq[a] for voxel (i0, i1, i2), the cell [i, i + 1);
 *   SPHERE (radius extent[0]): D0^2 + D1^2 + D2^2 <= (2 eq[0])^2;  BOX: |D[a]| <= 2 eq[a] on every axis.
 * A brush is invalid (RTO_E_INVALID) for an unknown shape or op, a NaN or infinite input, a negative extent, or |cq| or eq above
 * 2^27.  Brushes apply in array order (the later one wins); voxels outside the grid's dims do not exist, the grid never grows.
 * rto_edit_voxels: *changed (may be NULL) = voxels whose final value differs from their value before the call.  When it is > 0
 * the context is then as rto_build_octree(edited grid, same gridMin, same voxelSize) leaves it (nodes, descriptors, info, scene
 * bounds; frustum culling off), on the build path rto_debug_set_build_path chose, and leaf triangles that were resident are
 * rebuilt from the edited grid as rto_build_leaf_triangles(NULL) builds them.  changed == 0 touches nothing.  n == 0: no-op.
 * RTO_E_NO_OCTREE: no octree; RTO_E_UNSUPPORTED: the octree came from rto_upload_octree (no resident grid); RTO_E_INVALID: an
 * invalid brush, NULL brushes with n > 0, n < 0 or n > RTO_EDIT_MAX_BRUSHES.  Every error leaves the context untouched.
 * Synchronous on the context's stream. */
#define RTO_BRUSH_SPHERE 0
#define RTO_BRUSH_BOX    1
#define RTO_EDIT_CARVE   0   /* -> EMPTY  */
#define RTO_EDIT_FILL    1   /* -> FILLED */
#define RTO_EDIT_MAX_BRUSHES 65536
typedef struct rto_brush {          /* 32 bytes */
    float   centre[3];              /* world units */
    float   extent[3];              /* SPHERE: radius in extent[0] (extent[1..2] are checked, not used); BOX: half-sizes */
    int32_t shape;                  /* RTO_BRUSH_* */
    int32_t op;                     /* RTO_EDIT_* */
} rto_brush;

int  rto_edit_voxels(rto_context* ctx, const rto_brush* brushes, int n, int64_t* changed);
/* The resident grid, dims[2] x dims[1] x dims[0] bytes, x fastest (rto_build_octree's layout).  out == NULL: dims only (dims may
 * be NULL).  Errors as rto_edit_voxels; RTO_E_INVALID when capacity is below the grid's size. */
int  rto_download_voxels(rto_context* ctx, uint8_t* out, int64_t capacity, int dims[3]);
/* Device time in ms of the last rto_edit_voxels: the brush kernel, the octree rebuild, the triangle rebuild (-1: not run). */
int  rto_last_edit_ms(const rto_context* ctx, float ms[3]);
/* Pure host function, no device: the quantised brush of the rule above for this grid, or RTO_E_INVALID. */
int  rto_brush_quantize(const rto_brush* brush, const float grid_min[3], float voxel_size, int64_t cq[3], int64_t eq[3]);

/* ---- mesh voxelization ----------------------------------------------------
 * Builds the resident grid from a triangle mesh on the GPU, then the octree from it: the rule of the
 * reference's loadCSVDataIntoVoxelGrid (S/BuildingLoader.cpp:153-290), bit for bit.  xyz: n_verts rows x, y, z (double); tris:
 * n_tris faces of three row indices into xyz (the host layer, host/BuildingLoader.cpp, resolves the CSV's mesh and vertex numbers).
 *   grid (AUTO)   over the rows whose three coordinates are finite, in double: min / max, padded by (double)voxel_size on both
 *                 sides; dim = (size_t)ceil((max - min) / voxel_size).  If a dim exceeds 1000: scale = (float)max(dimX / 1000,
 *                 dimY / 1000, dimZ / 1000) in integer (size_t) division, voxel_size *= scale in float (a dim of 1001..1999 gives
 *                 scale 1: no change), and the dims are recomputed.  grid_min = (float)min.
 *   grid (FIXED)  params' dims, grid_min and voxel_size.
 *   per face      vertices rounded to float (a, b, c = rows tris[3f], tris[3f + 1], tris[3f + 2]); a face with a non-finite vertex is
 *                 skipped.  All float, one IEEE operation per operator: start = max(0, (int)((triMin - grid_min) / voxel_size)),
 *                 end = min(dim - 1, (int)((triMax - grid_min) / voxel_size) + 1) per axis, (int) truncating.  Each voxel i of
 *                 [start, end]^3 is FILLED when its centre p = grid_min + ((float)i + 0.5f) * voxel_size passes the reference's
 *                 isPointInTriangle (S/BuildingLoader.cpp:131-151): v0 = c - a, v1 = b - a, v2 = p - a, dot(x, y) = (x.x y.x +
 *                 x.y y.y) + x.z y.z, denom = d00 d11 - d01 d01, rejected when |denom| < 1e-7f, inv = 1.0f / denom,
 *                 u = (d11 d02 - d01 d12) inv, v = (d00 d12 - d01 d02) inv, inside when u >= 0 && v >= 0 && u + v <= 1.
 *                 The grid is the OR over faces (face order does not matter).  A prism test: the plane distance is bounded only
 *                 by the face's box.
 *   recentring    recenter_passes times (0..2; S/main.cpp:376-422 runs twice on the CSV path, :1039 and :1074): lo / hi = float
 *                 min / max over the FILLED voxels of their centres, grid_min -= 0.5f * (lo + hi); no FILLED voxel: no change.
 * On success the context is in the state rto_build_octree(grid, grid_min, voxel_size) leaves (nodes, descriptors, info, scene
 * bounds; frustum culling off; the grid kept resident, so rto_download_voxels, rto_edit_voxels and rto_build_leaf_triangles(NULL)
 * work), on the build path rto_debug_set_build_path chose; triangles != 0 then also builds the leaf triangles as
 * rto_build_leaf_triangles(NULL) does.  result (may be NULL) gets the grid after recentring.
 * RTO_E_INVALID: NULL params, n_verts or n_tris < 0, NULL xyz / tris with n > 0, a row index outside [0, n_verts), an unknown
 * mode, recenter_passes outside 0..2, a voxel_size that is not finite and positive, a FIXED grid with a dim below 1 or a non-finite
 * grid_min, a face whose (int) casts above would overflow (undefined in the reference), an AUTO grid that is empty (no face, or
 * no row with finite coordinates: the reference returns an empty grid, which rto_build_octree refuses), or a grid above the
 * build's size limit (a dim above 2^20).  Every error leaves the context untouched.  Synchronous on the context's stream. */
#define RTO_VOXELIZE_AUTO  0
#define RTO_VOXELIZE_FIXED 1
typedef struct rto_voxelize_params {   /* 40 bytes */
    int32_t mode;                      /* RTO_VOXELIZE_* */
    float   voxel_size;                /* AUTO: the requested size (the grid's may be scaled up); FIXED: the grid's */
    int32_t dims[3];                   /* FIXED only */
    float   grid_min[3];               /* FIXED only */
    int32_t recenter_passes;           /* 0, 1 or 2 */
    int32_t triangles;                 /* != 0: also build the leaf triangles */
} rto_voxelize_params;
typedef struct rto_voxelize_result {   /* 48 bytes */
    int32_t dims[3];
    float   grid_min[3];               /* after recentring */
    float   voxel_size;
    int32_t reserved;
    int64_t filled;                    /* FILLED voxels of the grid */
    int64_t pairs;                     /* (face, voxel) pairs tested: the voxels of the faces' boxes, degenerate faces excluded */
} rto_voxelize_result;

int  rto_voxelize_mesh(rto_context* ctx, const double* xyz, int64_t n_verts, const int32_t* tris, int64_t n_tris,
                       const rto_voxelize_params* params, rto_voxelize_result* result /* may be NULL */);
/* Device time in ms of the last rto_voxelize_mesh: face setup + scan, fill, recentring reduction, octree build (-1: not run). */
int  rto_last_voxelize_ms(const rto_context* ctx, float ms[4]);

/* ---- mesh extraction ------------------------------------------------------
 * The triangle list the reference's renderOctree (S/main.cpp:95-208) hands to its MarchingCubes and VoxelCube display modes, made
 * on the GPU from the resident octree.  All float32, one IEEE operation per operator.  Rule:
 *   visibility    a leaf is emitted when its own box and every ancestor's, up to the root, pass Frustum::testAABB(min, max, margin)
 *                 != -1 with min = gridMin + (float)xyz * voxelSize, max = min + (float)size * voxelSize (rto_update_frustum's
 *                 arithmetic).  Hierarchical: a leaf below a culled ancestor is dropped whatever its own test says.  cull == NULL:
 *                 every leaf is visible.  The state rto_update_frustum left is ignored, as in the queries.
 *   order         depth first, children in slots 0..7; within a leaf the extractor's own order.
 *   reach         the walk starts at node 0 and descends through nodes with isLeaf == 0 && isUniform == 0, as every traversal here
 *                 does: a node with isUniform == 1 && isLeaf == 0 ends it and emits nothing, and a leaf that the array holds but
 *                 the walk does not reach (below such a node, or an orphan) is not part of the mesh.
 *   RTO_MESH_MC   a visible leaf i contributes the resident leaf triangles tri_offset[i] .. tri_offset[i + 1], unchanged.
 *   RTO_MESH_CUBES  VoxelCubeRenderer::addBlockFaces (S/Renderer.cpp:64-98) on every visible leaf with isLeaf && isSolid: faces
 *                 +X, -X, +Y, -Y, +Z, -Z; a face is exposed when its ONE test voxel -- x0 + size (or x0 - 1) on the face's axis,
 *                 + size / 2 (integer) on the other two -- lies outside the grid's dims or is EMPTY in the resident grid.  The
 *                 reference tests the face's centre only, and so does this: a large leaf whose face centre is covered emits no
 *                 face.  Each face is two triangles (v0, v1, v3), (v3, v1, v2) of the corners S/Renderer.cpp:100-153 names, with
 *                 minCorner = gridMin + (float)x0 * voxelSize, maxCorner = minCorner + (float)size * voxelSize; the normal is the
 *                 axis unit vector with +0 zeros.
 * A record is 12 floats: v0, v1, v2, normal.  tri_node[j] = index, in the resident array, of the leaf that owns triangle j.
 * The result is a snapshot in a buffer the context owns: valid until the next rto_extract_mesh or rto_destroy, untouched by later
 * edits or builds.  Synchronous on the context's stream (one count is read back).  An empty result is RTO_OK with 0 triangles.
 * Errors, in this order, each leaving the previous mesh and the context untouched: RTO_E_INVALID (unknown kind, NULL num_tris, a
 * plane or margin that is not finite); RTO_E_NO_OCTREE (nothing uploaded); RTO_E_UNSUPPORTED (an array of more than one node that
 * is not canonical, or whose levels are not stored one after the other as setOctree's BFS and rto_build_octree store them); MC:
 * RTO_E_NO_OCTREE when no leaf triangles are resident; CUBES: RTO_E_UNSUPPORTED when no grid is resident (the octree came from
 * rto_upload_octree); RTO_E_UNSUPPORTED for more than 2^31 - 1 triangles. */
#define RTO_MESH_MC     0   /* MarchingCubesRenderer: the resident leaf triangles */
#define RTO_MESH_CUBES  1   /* VoxelCubeRenderer: exposed faces of the solid leaves */
typedef struct rto_mesh_cull {      /* 100 bytes */
    float planes[24];               /* LEFT, RIGHT, TOP, BOTTOM, NEAR, FAR as nx, ny, nz, d; normalised (rto_debug_update_frustum_planes' layout) */
    float margin;                   /* renderOctree's extraMargin; its default is 50 */
} rto_mesh_cull;

/* Pure host function: the planes rto_update_frustum derives, Frustum(perspective(radians(fov_deg), aspect, 0.01, 5000) * view)
 * (renderOctree builds its own the same way with fov 45, S/main.cpp:124-129). */
int  rto_frustum_planes(const float view[16], float fov_deg, float aspect, float planes[24]);
int  rto_extract_mesh(rto_context* ctx, int kind, const rto_mesh_cull* cull /* NULL: no culling */, int64_t* num_tris);
/* The last mesh where it lies: num_tris records of 48 bytes and as many int32 (both may be NULL for the count alone). */
int  rto_mesh_device(rto_context* ctx, void** d_tris, int32_t** d_tri_node, int64_t* num_tris);
/* Copies it out; tris == NULL and tri_node == NULL: the count alone.  RTO_E_INVALID: no mesh extracted yet, capacity too small. */
int  rto_download_mesh(rto_context* ctx, float* tris, int64_t capacity, int32_t* tri_node /* may be NULL */, int64_t* num_tris);
/* Device time in ms of the last rto_extract_mesh: count + cull, the ranking passes, the emit kernel (-1: not run).  The read-back
 * of the count and the growth of the output buffer lie between the last two and are in none of them. */
int  rto_last_mesh_ms(const rto_context* ctx, float ms[3]);

/* ---- lit render -----------------------------------------------------------
 * The box render's frame with a shadow ray and ambient occlusion per hit pixel, computed on the device in one stream (DESIGN.md
 * section 12).  Rule:
 *   primary hit   the FIRST box query on the frame's pixel ray (rto_render_device's rule, window (0, 1e30)): leaf, tHit =
 *                 max(0, tNear), entry face.  Like the queries, the lit render ignores rto_update_frustum.
 *   ndotl         shade_term's Lambert term against lightNeg = -normalize(light_dir), normalised as the renders do.
 *   origin        a = face >> 1, sigma = +1 if (face & 1) else -1 (sigma e_a is the entry face's outward normal); p = o + d tHit;
 *                 eps = voxelSize * 1e-3f + 2^-18 * max(|p.x|, |p.y|, |p.z|); so = p except so[a] = the leaf's float plane on axis
 *                 a (max plane if sigma > 0, min plane otherwise) + sigma eps.
 *   shadow        (shadow != 0, face >= 0, ndotl > 0) one ray from so towards lightNeg, window (0, 1e30), the ANY rule: S = 0 when it
 *                 hits, else 1.
 *   AO            (K = ao_samples in 1..64, face >= 0) K rays from so, window (0, ao_radius], the ANY rule.  T = rto_ao_directions
 *                 (64 unit vectors, z > 0, cosine-weighted Hammersley); h = mix32(x * 0x8da6b343 ^ y * 0xd8163841 ^ seed * 0xcb1ab31f)
 *                 in uint32, mix32(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16.  Sample s uses
 *                 t = T[(h + (64 s) / K) & 63]; the world direction has component a = sigma t.z, component (a + 1) % 3 = t.x negated
 *                 when bit 6 of h is set, component (a + 2) % 3 = t.y negated when bit 7 is set.  occ = rays that hit;
 *                 A = (float)(K - occ) / (float)K.
 *   otherwise     S = A = 1 (K = 0, no shadow ray cast, or face = -1: the camera inside a solid leaf).
 *   colour        d = S ? ndotl : 0, amb = 0.1f * A, RGBA = (1.0f d + amb, 0.8f d + amb, 0.6f d + amb, 1); a miss is (0, 0, 0, 1).
 *                 shadow = 0, K = 0 and light_dir = (-1, -1, -1) give rto_render_device's frame (culling off) bit for bit.
 *   vis           (optional, int32 per pixel) -1 for a miss, else occ + 256 * (shadow ray cast and blocked).
 * Whole frames only.  RTO_E_INVALID: a NULL frame, lighting or output, a misaligned device buffer (d_rgba 16 bytes, d_vis 4), K
 * outside 0..64, K > 0 with an ao_radius that is not finite and positive, a light_dir that is zero, not finite or not normalisable
 * in float, reserved != 0, a width or height below 1, or a frame too large for 32-bit ray indices: width * height * (K + 1) + 128
 * and 64 * (8x8 tiles of the frame) + 256 must both be below 2^32; RTO_E_NO_OCTREE: nothing uploaded; RTO_E_UNSUPPORTED: an array
 * of more than one node without a descriptor tree (a non-canonical upload).  A tree that is one leaf is rendered (its box is the
 * walk).  rto_set_kernel does not apply.  The device form is asynchronous on hip_stream and keeps its work buffers
 * on the context (a frame larger than any before allocates them, and then must not be stream-captured; one set per context, so
 * lit frames on different streams of one context must not run at the same time). */
#define RTO_AO_MAX_SAMPLES 64
typedef struct rto_lighting {       /* 32 bytes */
    float    light_dir[3];          /* direction the light travels; (-1, -1, -1) is the renders' light */
    int32_t  shadow;                /* != 0: cast the shadow ray */
    int32_t  ao_samples;            /* K, 0..RTO_AO_MAX_SAMPLES */
    float    ao_radius;             /* AO window's t_max, world units (the directions are unit vectors) */
    uint32_t seed;
    int32_t  reserved;              /* 0 */
} rto_lighting;

int  rto_render_lit_device(rto_context* ctx, const rto_frame* frame, const rto_lighting* lighting, void* d_rgba,
                           int32_t* d_vis /* may be NULL */, void* hip_stream);
int  rto_render_lit_host(rto_context* ctx, const rto_frame* frame, const rto_lighting* lighting, float* host_rgba,
                         int32_t* host_vis /* may be NULL */);
/* The 64 AO directions T (x, y, z per entry): entry i is u = (i + 0.5) / 64, phi = 2 pi (bitrev6(i) + 0.5) / 64,
 * (sqrt(u) cos phi, sqrt(u) sin phi, sqrt(1 - u)) computed in double and rounded once to float.  Pure host function. */
int  rto_ao_directions(float out[192]);

/* ---- lit render of the triangle surface -----------------------------------
 * rto_render_triangles_device's frame with a shadow ray and ambient occlusion per hit pixel, computed on the device in one stream
 * (DESIGN.md section 14): the lit render above on the resident leaf triangles.  rto_lighting is the lit render's.  All arithmetic
 * is float32, one IEEE operation per operator, in the order written; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.  Rule:
 *   primary hit   the FIRST triangle query on the frame's pixel ray, window (0, 1e30): rto_query_triangle_pixels_*'s record (t,
 *                 triangle, owning leaf, u, v, and n = the stored face normal, negated when dot(n, d) > 0).  This is
 *                 rto_render_triangles_device's hit.  Like the queries, the frame ignores rto_update_frustum.
 *   ndotl         max(0, dot(n, lightNeg)), glm's max ((a < b) ? b : a), lightNeg = -normalize(light_dir) as rto_render_lit_* has it.
 *   origin        p = o + d t; eps = voxelSize * 1e-3f + 2^-18 * max(|p.x|, |p.y|, |p.z|); h = eps - dot(p - v0, n) with v0 the
 *                 triangle's first vertex; so = p + n h (the triangle render's shadow origin).  Shadow and AO rays start there.
 *   shadow        (shadow != 0, ndotl > 0) one ray from so along lightNeg, window (0, 1e30), the ANY triangle rule: S = 0 when it
 *                 hits, else 1.
 *   AO            (K = ao_samples in 1..64) K rays from so, window (0, ao_radius], the ANY triangle rule.  T, h and the entry
 *                 t = T[(h + (64 s) / K) & 63] of sample s are the lit render's; x' = t.x negated when bit 6 of h is set, y' = t.y
 *                 negated when bit 7 is set, z' = t.z.  The frame around n (Duff et al., "Building an Orthonormal Basis,
 *                 Revisited"): s = (n.z < 0) ? -1 : 1; a = -1 / (s + n.z); b = (n.x * n.y) * a;
 *                 U = (1 + ((s * n.x) * n.x) * a, s * b, (-s) * n.x); V = (b, s + (n.y * n.y) * a, -n.y); per component c:
 *                 dir[c] = (x' * U[c] + y' * V[c]) + z' * n[c].  The direction is not renormalised (a stored normal is unit only
 *                 to rounding) and the window is in the ray's own parameter, as in every query.  occ = rays that hit;
 *                 A = (float)(K - occ) / (float)K.
 *   misses        a shadow or AO ray whose origin or direction has a NaN or infinite component is a miss (stored normals that
 *                 are zero, huge or not finite are accepted input).
 *   otherwise     S = A = 1 (K = 0, no shadow ray cast).
 *   colour, vis   the lit render's: d = S ? ndotl : 0, amb = 0.1f * A, RGBA = (1.0f d + amb, 0.8f d + amb, 0.6f d + amb, 1); a miss
 *                 is (0, 0, 0, 1); vis = -1 for a miss, else occ + 256 * (shadow ray cast and blocked).
 * shadow = 0, K = 0 and light_dir = (-1, -1, -1) give rto_render_triangles_device(shadow = 0)'s frame (culling off) bit for bit;
 * shadow = 1, K = 0 gives its shadow = 1 frame on every pixel whose shadow ray has the same verdict under FIRST (the render's walk,
 * with its 512-pop cap) and ANY (no cap).
 * Whole frames only.  The errors are rto_render_lit_*'s, checked first and in its order (RTO_E_INVALID, RTO_E_NO_OCTREE: nothing
 * uploaded, RTO_E_UNSUPPORTED: a non-canonical array of more than one node), then RTO_E_NO_OCTREE when no leaf triangles are
 * resident (rto_build_leaf_triangles / rto_upload_leaf_triangles).  A tree that is one leaf owns no triangles: every pixel is a
 * miss.  rto_set_kernel does not apply.  The device form is asynchronous on hip_stream and shares the lit render's work buffers
 * on the context (same rules: a frame larger than any before allocates them and must not be stream-captured; lit frames of either
 * kind on different streams of one context must not run at the same time). */
int  rto_render_lit_triangles_device(rto_context* ctx, const rto_frame* frame, const rto_lighting* lighting, void* d_rgba,
                                     int32_t* d_vis /* may be NULL */, void* hip_stream);
int  rto_render_lit_triangles_host(rto_context* ctx, const rto_frame* frame, const rto_lighting* lighting, float* host_rgba,
                                   int32_t* host_vis /* may be NULL */);

/* ---- region queries ---------------------------------------------------------
 * Questions about a place instead of a ray: which leaf holds a point, how much solid a brush covers, how far the nearest solid
 * is.  No reference counterpart as an API: the click handler (S/main.cpp:646-700) answers the first by a CPU march over the dense
 * grid.  Every result is an integer that a brute-force count over the grid reproduces bit for bit.
 *
 * Rule, exact in integers at 1/64 voxel, the voxel edits' quantisation:
 *   point     pq[a] = floor((p[a] - gridMin[a]) / voxelSize * 64 + 0.5), in double from the context's float gridMin / voxelSize
 *             (rto_point_quantize).  Invalid: a NaN or infinite component, or |pq[a]| > 2^27.
 *   region    an rto_brush; cq, eq as rto_brush_quantize gives them.  Invalid exactly when rto_brush_quantize refuses the brush
 *             with its `op` field set to RTO_EDIT_CARVE: the op is ignored.
 *   invalid   records are marked in the output (below) and never make the call fail, as NaN rays are misses in the ray queries.
 *   reach     the walk starts at node 0 and descends through nodes with isLeaf == 0 && isUniform == 0; every other node it meets
 *             is a leaf, solid when isSolid == 1.  A leaf the walk does not reach does not exist.  rto_update_frustum is ignored.
 *             A child's box lies inside its parent's (every octree; an uploaded array that breaks this is walked as if it held:
 *             a subtree is dropped when its root's box is out of the question's reach).
 *   dims      the domain: with a resident grid (rto_build_octree, rto_voxelize_mesh, after rto_edit_voxels) that grid's dims,
 *             [0, dims[a]) per axis; for an octree from rto_upload_octree the cube [x, x + size) of node 0 on each axis.
 * Point location: voxel i[a] = pq[a] >> 6 (floor).  The answer is the reached leaf whose box [x, x + size) holds i on every axis;
 *   where several do (a non-canonical array) the lowest node index wins.
 * Brush census: voxel (i0, i1, i2) is covered exactly when the edit rule says the brush touches it: D[a] = 64 (2 i[a] + 1) -
 *   2 cq[a]; SPHERE: D0^2 + D1^2 + D2^2 <= (2 eq[0])^2; BOX: |D[a]| <= 2 eq[a] on every axis; all in int64.  On an octree built
 *   from a grid, filled = the FILLED covered voxels of rto_download_voxels, a CARVE of the brush reports changed == filled and a
 *   FILL changed == covered - filled.  (filled < 2^63 always: the domain holds at most 2^60 voxels of an octree of depth 20.)
 * Nearest solid: mq = floor(max_dist / voxelSize * 64 + 0.5) in double; the record is invalid when the point is, when max_dist
 *   is NaN or negative, or when mq > 2^28; max_dist = +inf is no limit.  A reached solid leaf's box in 1/64 units is
 *   [64 x, 64 (x + size)] per axis, closed; c[a] = clamp(pq[a], lo, hi), dist2 = sum (pq[a] - c[a])^2 in int64.  The answer is the
 *   least dist2 with dist2 <= mq^2, ties to the lowest node index.  dist2 == 0 exactly when pq lies in a closed solid box.
 * Alignment (16 bytes, every buffer), n == 0 and the error codes are those of rto_query_rays_*: RTO_E_INVALID for a NULL buffer,
 * n < 0 or a misaligned buffer, RTO_E_NO_OCTREE for nothing uploaded.  Every octree the ray queries accept is accepted: a tree that
 * is one leaf, non-canonical arrays.  _device: asynchronous on hip_stream, device buffers, allocates nothing.  _host: synchronous,
 * host buffers.  rto_set_kernel does not apply.
 * Cost: a partly covered SPHERE region is counted row by row (one integer square root per row of voxels along x), so a sphere
 * costs its cross-section in rows where it cuts a solid leaf or the domain's faces; everything else is closed form. */
typedef struct rto_point_hit {      /* 32 bytes */
    int32_t node;                   /* index in the resident array; -1: outside every reached leaf, or an invalid point */
    int32_t solid;                  /* 1 when that leaf is solid; 0 otherwise and for node == -1 */
    int32_t x, y, z, size;          /* the leaf's box, voxel units; 0 for node == -1 */
    int32_t depth;                  /* levels below the root (nodes descended through) */
    int32_t reserved;               /* 0 */
} rto_point_hit;

typedef struct rto_region {         /* 32 bytes */
    int64_t filled;                 /* covered voxels inside reached solid leaves (each leaf's box clipped to dims); -1: invalid */
    int64_t covered;                /* covered voxels inside dims; -1: invalid */
    int32_t solid_leaves;           /* reached solid leaves holding at least one covered voxel inside dims */
    int32_t first_node;             /* the lowest index among them; -1: none */
    int32_t reserved[2];            /* 0 */
} rto_region;

typedef struct rto_near_point {     /* 16 bytes: the input of the nearest-solid query */
    float x, y, z, max_dist;        /* world units; max_dist >= 0, +inf: no limit */
} rto_near_point;

typedef struct rto_nearest {        /* 32 bytes */
    int64_t dist2;                  /* squared distance in 1/64-voxel units; -1: no solid within max_dist, or invalid */
    int32_t node;                   /* the solid leaf; -1 with dist2 == -1 */
    int32_t size;                   /* its size, voxel units; 0 with dist2 == -1 */
    int32_t cq[3];                  /* the closest point c of its closed box, 1/64-voxel units; 0 with dist2 == -1 */
    int32_t reserved;               /* 0 */
} rto_nearest;

/* points: n records of 3 floats (x, y, z), 12 bytes each; the buffer 16-byte aligned. */
int  rto_query_points_device(rto_context* ctx, const float* d_points, int64_t n, rto_point_hit* d_hits, void* hip_stream);
int  rto_query_points_host(rto_context* ctx, const float* points, int64_t n, rto_point_hit* hits);
int  rto_query_regions_device(rto_context* ctx, const rto_brush* d_brushes, int64_t n, rto_region* d_regions, void* hip_stream);
int  rto_query_regions_host(rto_context* ctx, const rto_brush* brushes, int64_t n, rto_region* regions);
int  rto_query_nearest_device(rto_context* ctx, const rto_near_point* d_points, int64_t n, rto_nearest* d_out, void* hip_stream);
int  rto_query_nearest_host(rto_context* ctx, const rto_near_point* points, int64_t n, rto_nearest* out);
/* Pure host function, no device: pq of the rule above for this grid; RTO_E_INVALID for an invalid point, a NULL argument or a
 * voxel_size that is not finite and positive. */
int  rto_point_quantize(const float p[3], const float grid_min[3], float voxel_size, int64_t pq[3]);

/* ---- connected components -------------------------------------------------
 * Labels the resident grid (rto_build_octree, rto_voxelize_mesh, after edits) and flips whole components: debris left floating by
 * a carve, the cavity inside a voxelized shell.  No reference counterpart.  Every result is an integer that a brute-force
 * flood fill over rto_download_voxels reproduces bit for bit.
 *
 * Rule:
 *   index     voxel (i, j, k) has linear index v = i + dimX (j + dimY k): rto_download_voxels' layout.
 *   set       RTO_SET_SOLID: the voxels equal to 1; RTO_SET_EMPTY: the voxels equal to 0.  Voxels outside the grid do not exist:
 *             they belong to no set and connect nothing.
 *   joined    RTO_CONN_FACE (6): two voxels of the set that differ by 1 on exactly one axis; RTO_CONN_FULL (26): two that differ by
 *             at most 1 on every axis and are not equal.  Components are the classes of the transitive closure.
 *   canonical a component's root is the smallest linear index among its voxels; components are numbered 0 .. count - 1 in
 *             ascending order of root; the label volume holds that number for voxels of the set and -1 for the others.  Nothing
 *             depends on scheduling.
 * rto_label_components keeps the label volume (int32 per voxel) and the table resident; they describe the grid they were made
 * from, and every call that changes or replaces the grid frees them (rto_build_octree, rto_upload_octree, rto_voxelize_mesh,
 * rto_edit_voxels / rto_edit_components with changed > 0, rto_destroy): the readers then return RTO_E_INVALID.  An empty set
 * gives count 0, a volume of -1 and an empty table.  Synchronous on the context's stream.
 * rto_edit_components labels afresh (the resident labels are not consulted), selects components, and flips every voxel of the
 * selected ones (SOLID -> 0, EMPTY -> 1).  *changed (may be NULL) = voxels flipped.  When it is > 0 the context is left exactly as
 * rto_edit_voxels leaves it after a change (rebuild on the build path in force, resident leaf triangles rebuilt, frustum culling
 * off); changed == 0 touches nothing.
 *   RTO_SELECT_SMALLER_THAN      voxels < arg
 *   RTO_SELECT_ALL_BUT_LARGEST   every component except the one with the most voxels; on a tie the smaller root is kept
 *   RTO_SELECT_ENCLOSED          touches == 0
 *   RTO_SELECT_CONTAINING        the component that holds linear voxel arg; none if that voxel is not in the set
 *   RTO_SELECT_NOT_CONTAINING    all but that one; none if that voxel is not in the set
 * Errors, each leaving the context untouched: RTO_E_INVALID (unknown set, connectivity or selection; arg < 0 for SMALLER_THAN and
 * the CONTAINING forms; arg at or beyond the voxel count for the CONTAINING forms; too small a capacity; no resident labels);
 * RTO_E_NO_OCTREE (no octree built); RTO_E_UNSUPPORTED (the octree came from rto_upload_octree: no resident grid; or the grid
 * has more than 2^31 - 2 voxels: labels are 32-bit); RTO_E_INTERNAL (merging did not settle in 32 passes: a defect). */
#define RTO_SET_SOLID 1
#define RTO_SET_EMPTY 0
#define RTO_CONN_FACE 6
#define RTO_CONN_FULL 26
#define RTO_SELECT_SMALLER_THAN    0
#define RTO_SELECT_ALL_BUT_LARGEST 1
#define RTO_SELECT_ENCLOSED        2
#define RTO_SELECT_CONTAINING      3
#define RTO_SELECT_NOT_CONTAINING  4
typedef struct rto_component {      /* 48 bytes */
    int64_t root;                   /* smallest linear voxel index of the component */
    int64_t voxels;                 /* its size */
    int32_t lo[3], hi[3];           /* inclusive voxel bounding box */
    int32_t touches;                /* bit a: has a voxel with index 0 on axis a; bit 3 + a: one with index dim[a] - 1 */
    int32_t reserved;               /* 0 */
} rto_component;

int  rto_label_components(rto_context* ctx, int set, int connectivity, int64_t* count /* may be NULL */);
/* out == NULL: the count alone. */
int  rto_download_components(rto_context* ctx, rto_component* out, int64_t capacity, int64_t* count);
/* dimZ x dimY x dimX int32, x fastest. */
int  rto_download_labels(rto_context* ctx, int32_t* out, int64_t capacity);
/* The resident label volume and table (device pointers the context owns, valid until the labels are freed). */
int  rto_labels_device(rto_context* ctx, int32_t** d_labels, rto_component** d_components, int64_t* count);
/* Device time in ms of the last rto_label_components: tile-local labelling, merging (all passes, with the host's look at the
 * flag between them), flatten + ranking + label volume, statistics (-1: not run). */
int  rto_last_components_ms(const rto_context* ctx, float ms[4]);
/* Merge launches of the last rto_label_components (2 = one merge and one clean check; the cap is 32). */
int  rto_debug_components_passes(const rto_context* ctx, int* passes);
int  rto_edit_components(rto_context* ctx, int set, int connectivity, int select, int64_t arg, int64_t* changed /* may be NULL */);

/* ---- distance fields and morphology -----------------------------------------
 * How far every voxel of the resident grid is from a set of its voxels, exactly, and the edits that move the surface by a distance:
 * thicken a voxelized shell until rto_edit_components can see it as closed, close pinholes, open away attached whiskers, find the
 * thickest point of a part.  No reference counterpart.  Every result is an integer that a brute-force minimum over
 * rto_download_voxels reproduces bit for bit.
 *
 * Rule:
 *   index     voxel (i, j, k) has linear index v = i + dimX (j + dimY k); the sets are rto_label_components': RTO_SET_SOLID the
 *             voxels equal to 1, RTO_SET_EMPTY the voxels equal to 0.  Voxels outside the grid belong to no set.
 *   field     d2[v] = min over the voxels u of the set of (i_v - i_u)^2 + (j_v - j_u)^2 + (k_v - k_u)^2, as int32, in voxel-index
 *             units (multiply by voxelSize^2 for world units): 0 exactly on the set; RTO_DIST_NONE where the set is empty.  No
 *             nearest-voxel index is returned: ties would need a rule the separable passes do not give for free.
 *   cap       mq = floor(max_dist / voxelSize * 64 + 0.5) in double from the context's floats, as rto_query_nearest_* quantises
 *             max_dist; +inf: no cap.  A voxel is in reach when 4096 d2 <= mq^2 (int64); voxels out of reach hold RTO_DIST_NONE,
 *             so a capped field is the uncapped one, thresholded.
 *   summary   max_d2 the largest finite value, argmax the smallest linear index that holds it, finite the number of finite
 *             values; max_d2 = argmax = -1 when finite is 0.
 * rto_distance_field keeps the volume (int32 per voxel) resident; it describes the grid it was made from, and every call that
 * changes or replaces the grid frees it (rto_build_octree, rto_upload_octree, rto_voxelize_mesh, rto_edit_voxels /
 * rto_edit_components / rto_edit_morphology with changed > 0, rto_destroy): the readers then return RTO_E_INVALID.  Synchronous on
 * the context's stream.
 * rto_edit_morphology quantises radius to rq as max_dist is quantised to mq and makes its own capped fields (the resident one is
 * not consulted):
 *   RTO_MORPH_DILATE   an EMPTY voxel becomes FILLED when its d2 to SOLID is in reach of rq
 *   RTO_MORPH_ERODE    a FILLED voxel becomes EMPTY when its d2 to EMPTY is in reach
 *   RTO_MORPH_OPEN     ERODE, then DILATE of the result;   RTO_MORPH_CLOSE   DILATE, then ERODE of the result
 * The outside of the grid is no set: erosion never eats in from the grid's faces and dilation never grows past them, so on the
 * subsets of the grid dilate(X) is inside Y exactly when X is inside erode(Y); CLOSE only adds, OPEN only removes, both are
 * idempotent.  The DILATE by r of a single FILLED voxel is the voxel set of rto_edit_voxels' FILL with a SPHERE brush of radius r
 * on that voxel's centre.  *changed (may be NULL) = voxels whose final value differs from their value before the call (for OPEN
 * and CLOSE: from the grid before the first step).  When it is > 0 the context is left exactly as rto_edit_voxels leaves it after a
 * change (one rebuild on the build path in force, resident leaf triangles rebuilt, frustum culling off, labels and field freed);
 * changed == 0 (rq == 0 included) touches nothing.
 * Errors, each leaving the context untouched: RTO_E_INVALID (unknown set or op; max_dist or radius NaN, negative, or beyond 2^28
 * quanta; too small a capacity; no resident field); RTO_E_NO_OCTREE (no octree built); RTO_E_UNSUPPORTED (the octree came from
 * rto_upload_octree: no resident grid; more than 2^31 - 2 voxels; (dimX-1)^2 + (dimY-1)^2 + (dimZ-1)^2 >= 2^31 - 1: the field is
 * 32-bit -- 46342 x 1 x 1 is refused, 46341 x 1 x 1 accepted). */
#define RTO_DIST_NONE 0x7fffffff
#define RTO_MORPH_DILATE 0
#define RTO_MORPH_ERODE  1
#define RTO_MORPH_OPEN   2
#define RTO_MORPH_CLOSE  3
typedef struct rto_dist_summary {   /* 32 bytes */
    int64_t max_d2;                 /* the largest finite value; -1: none */
    int64_t argmax;                 /* the smallest linear voxel index that holds it; -1: none */
    int64_t finite;                 /* voxels with a finite value */
    int64_t reserved;               /* 0 */
} rto_dist_summary;

int  rto_distance_field(rto_context* ctx, int set, float max_dist, rto_dist_summary* summary /* may be NULL */);
/* dimZ x dimY x dimX int32, x fastest. */
int  rto_download_distance(rto_context* ctx, int32_t* out, int64_t capacity);
/* The resident field (a device pointer the context owns, valid until the field is freed). */
int  rto_distance_device(rto_context* ctx, int32_t** d_d2);
/* Device time in ms of the last rto_distance_field: x pass, y pass, z pass, summary (-1: not run). */
int  rto_last_distance_ms(const rto_context* ctx, float ms[4]);
int  rto_edit_morphology(rto_context* ctx, int op, float radius, int64_t* changed /* may be NULL */);
/* Device time in ms of the last rto_edit_morphology: transforms and flips, octree rebuild, triangle rebuild (-1: not run). */
int  rto_last_morphology_ms(const rto_context* ctx, float ms[3]);

/* ---- geodesic distance fields, paths and flood edits ----------------------------
 * How far every voxel of the resident grid is from a set of seed voxels along the way one can actually go: through free space
 * round the walls, or inside the material.  Which voxels a spill, a crowd or a tool reaches within a number of steps, how thick
 * the material is between two points measured inside it, by which route a target is reached.  No reference counterpart.  Every
 * result is an integer that a Dijkstra search over rto_download_voxels reproduces bit for bit.
 *
 * Rule:
 *   index     voxel (i, j, k) has linear index v = i + dimX (j + dimY k); the sets are rto_label_components': RTO_SET_SOLID the
 *             voxels equal to 1, RTO_SET_EMPTY the voxels equal to 0.  Voxels outside the grid do not exist.
 *   medium    the set the path stays in: RTO_SET_EMPTY free space, RTO_SET_SOLID through the material.
 *   moves     RTO_CONN_FACE: the 6 face neighbours, weight 1 (the value is a number of steps).  RTO_CONN_FULL: the 26
 *             neighbours, weight 3, 4, 5 for a move that changes 1, 2, 3 coordinates (the 3-4-5 chamfer: divide by 3 for voxel
 *             units).  A move needs both ends in the medium and nothing else: a diagonal move between two medium voxels is
 *             allowed whatever the voxels beside it hold, exactly as rto_label_components joins them, so the voxels in reach are
 *             the components of the medium, under the same connectivity, that hold a seed.
 *   seeds     n >= 1 linear indices, on the host.  A seed outside [0, voxels) is RTO_E_INVALID; a seed that is not in the
 *             medium is ignored; duplicates are allowed.
 *   field     g[v] = the smallest total weight of a path of moves from any seed to v, as int32: 0 on the seeds that lie in the
 *             medium; RTO_DIST_NONE outside the medium, where no seed reaches, and beyond the limit.
 *   limit     in the metric's own units; limit >= 0x7fffffff: none.  A voxel with g > limit holds RTO_DIST_NONE, so a limited
 *             field is the unlimited one, thresholded.
 *   summary   max_g the largest finite value, argmax the smallest linear index that holds it, reached the number of finite
 *             values; max_g = argmax = -1 when reached is 0.
 *   paths     on the resident field, under the connectivity it was made with.  From a target t with finite g[t] the path is
 *             t = p0, p1, ..., pm with g[pm] = 0, where p(k+1) is the smallest linear index among the neighbours u of pk with
 *             g[u] finite and g[u] + w(u, pk) == g[pk] (one always exists, in a limited field too); len = m + 1.  A target whose
 *             g is RTO_DIST_NONE has len = -1.  Row i of out_voxels (max_len entries) takes the first min(len, max_len) voxels
 *             of target i's path, -1 behind them; out_len[i] is always the full len, so max_len = 0 with out_voxels = NULL asks
 *             for lengths alone.
 *   flood     rto_edit_geodesic makes its own field (the resident one is not consulted) and flips every voxel with finite g:
 *             medium EMPTY becomes FILLED, medium SOLID becomes EMPTY.  *changed (may be NULL) = voxels flipped.  When it is > 0
 *             the context is left exactly as rto_edit_voxels leaves it after a change (one rebuild on the build path in force,
 *             resident leaf triangles rebuilt, frustum culling off, labels and both fields freed); changed == 0 (no seed in the
 *             medium, for example) touches nothing.  With no limit and one seed it is
 *             rto_edit_components(medium, connectivity, RTO_SELECT_CONTAINING, seed).
 * rto_geodesic_field keeps the volume (int32 per voxel) resident, beside the Euclidean field of rto_distance_field (both may be
 * resident); it describes the grid it was made from, and every call that changes or replaces the grid frees it, as it frees the
 * labels and the Euclidean field: the readers and rto_geodesic_paths then return RTO_E_INVALID.  Synchronous on the context's
 * stream.
 * Errors, each leaving the context untouched: RTO_E_INVALID (unknown medium or connectivity; n < 1; NULL seeds or targets; a seed
 * or target out of range; limit < 0; max_len < 0; too small a capacity; no resident geodesic field, for the readers and for
 * paths); RTO_E_NO_OCTREE (no octree built); RTO_E_UNSUPPORTED (the octree came from rto_upload_octree: no resident grid; more
 * than 2^31 - 2 voxels; w_max (voxels - 1) >= 2^31 - 1 with w_max 1 or 5: the field is 32-bit); RTO_E_INTERNAL (the relaxation
 * did not settle within voxels + 2 passes: a shortest path crosses tile boundaries fewer times than it has voxels). */
typedef struct rto_geo_summary {    /* 32 bytes */
    int64_t max_g;                  /* the largest finite value; -1: none */
    int64_t argmax;                 /* the smallest linear voxel index that holds it; -1: none */
    int64_t reached;                /* voxels with a finite value */
    int64_t reserved;               /* 0 */
} rto_geo_summary;

int  rto_geodesic_field(rto_context* ctx, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit,
                        rto_geo_summary* summary /* may be NULL */);
/* dimZ x dimY x dimX int32, x fastest. */
int  rto_download_geodesic(rto_context* ctx, int32_t* out, int64_t capacity);
/* The resident field (a device pointer the context owns, valid until the field is freed). */
int  rto_geodesic_device(rto_context* ctx, int32_t** d_g);
/* out_voxels: n rows of max_len int64 (may be NULL when max_len is 0); out_len: n int64.  Both on the host. */
int  rto_geodesic_paths(rto_context* ctx, const int64_t* targets, int64_t n, int64_t max_len, int64_t* out_voxels, int64_t* out_len);
int  rto_edit_geodesic(rto_context* ctx, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit,
                       int64_t* changed /* may be NULL */);
/* Device time in ms of the last rto_geodesic_field: init, relaxation (all passes, with the host's looks at the device), summary
 * (-1: not run). */
int  rto_last_geodesic_ms(const rto_context* ctx, float ms[3]);
/* Device time in ms of the last rto_edit_geodesic: field and flip, octree rebuild, triangle rebuild (-1: not run). */
int  rto_last_geodesic_edit_ms(const rto_context* ctx, float ms[3]);
/* The last rto_geodesic_field: relaxation launches up to and including the first that found no tile to run (at least 2: the tiles
 * that hold a seed always run once), and the tiles run summed over them (may be NULL). */
int  rto_debug_geodesic_passes(const rto_context* ctx, int64_t* passes, int64_t* tiles_run);
/* How many relaxation launches go out between two looks of the host at the device (1 .. 64, 8 by default).  A tuning choice: no
 * value of any field, path or edit depends on it. */
int  rto_debug_set_geodesic_look(rto_context* ctx, int passes_per_look);

/* ---- local thickness fields ---------------------------------------------------
 * How thick the material, or how wide the free space, is at every voxel of the resident grid: the largest ball that fits inside
 * the medium and contains the voxel (Hildebrand and Ruegsegger's local thickness), for balls up to a caller's radius of at most 8
 * voxels.  Which walls of a voxelized mesh are thinner than three voxels, where the narrowest gap between two buildings is, what the
 * pore-size distribution of the free space is.  rto_distance_field does not say: a voxel beside the surface of a thick part has
 * d2 = 1 exactly like a voxel of a one-voxel wall.  No reference counterpart.  Every result is an integer that a brute-force loop
 * over rto_download_voxels reproduces bit for bit.
 *
 * Rule:
 *   index     voxel (i, j, k) has linear index v = i + dimX (j + dimY k); the sets are rto_label_components': RTO_SET_SOLID the
 *             voxels equal to 1, RTO_SET_EMPTY the voxels equal to 0.  Voxels outside the grid do not exist.
 *   medium    RTO_SET_SOLID measures the material (wall thickness), RTO_SET_EMPTY the free space (pore width, clearance).
 *   cap       mq = floor(max_radius / voxelSize * 64 + 0.5) as rto_distance_field quantises max_dist; c = floor(mq^2 / 4096).
 *             c = 0 is RTO_E_INVALID (a radius under one voxel measures nothing); c > 64, +inf included, is RTO_E_UNSUPPORTED
 *             (more than 8 voxels).  The cap is part of the rule, not an approximation of another rule.
 *   radius    for a voxel q of the medium D[q] = min(d2 from q to the nearest voxel of the other set, c), d2 by
 *             rto_distance_field's rule with set = the complement of the medium; RTO_DIST_NONE (the other set is empty) clips
 *             to c.  D = 0 for a voxel outside the medium.
 *   field     for a voxel p of the medium t2[p] = max{ D[q] : q in the grid, (p - q)^2 < D[q] }, as int32; 0 for every other
 *             voxel.  The ball is open and q = p always qualifies, so a medium voxel holds at least 1 and at least its own D.
 *             A value below c is an exact width: a wall w voxels wide holds min(((w + 1) div 2)^2, c) throughout.  The value c
 *             reads "a ball of squared radius c fits here, or something larger".  The capped field is NOT min(uncapped field, c):
 *             a voxel covered only by a far larger ball whose centre is more than sqrt(c) away can come out lower (never higher).
 *   histogram bins[t], t = 0 .. c, int64: the number of medium voxels with t2 = t; bins[0] = 0; the sum is the number of medium
 *             voxels.  Made by every call and kept on the host in the context.
 *   summary   min_t2 the smallest value over the medium, argmin the smallest linear index that holds it, thin the number of
 *             medium voxels with t2 < c, medium the number of medium voxels; -1, -1, 0, 0 with no medium voxel.
 * rto_thickness_field keeps the volume (int32 per voxel) resident beside the labels, the Euclidean field and the geodesic field,
 * with its medium and its c; every call that changes or replaces the grid frees it as it frees them, and the readers then return
 * RTO_E_INVALID.  The call makes a private capped transform and frees it: a resident Euclidean field is neither read nor
 * replaced.  Synchronous on the context's stream.
 * Errors, in rto_distance_field's order, each leaving the context untouched: RTO_E_INVALID (unknown medium; max_radius NaN,
 * negative, beyond 2^28 quanta, or under one voxel; too small a capacity; no resident thickness field, for the readers);
 * RTO_E_UNSUPPORTED (max_radius above 8 voxels; no resident grid; a grid rto_distance_field refuses); RTO_E_NO_OCTREE. */
#define RTO_THICK_MAX_C 64          /* the largest c: balls of up to 8 voxels */
typedef struct rto_thick_summary {  /* 32 bytes */
    int64_t min_t2;                 /* the smallest value over the medium; -1: no medium voxel */
    int64_t argmin;                 /* the smallest linear voxel index that holds it; -1: none */
    int64_t thin;                   /* medium voxels with t2 < c */
    int64_t medium;                 /* medium voxels */
} rto_thick_summary;

int  rto_thickness_field(rto_context* ctx, int medium, float max_radius, rto_thick_summary* summary /* may be NULL */);
/* dimZ x dimY x dimX int32, x fastest. */
int  rto_download_thickness(rto_context* ctx, int32_t* out, int64_t capacity);
/* The resident field (a device pointer the context owns, valid until the field is freed). */
int  rto_thickness_device(rto_context* ctx, int32_t** d_t2);
/* The resident field's histogram: out takes c + 1 values (capacity >= c + 1; NULL: ask for *bins alone), *bins = c + 1 (may be
 * NULL).  Both on the host. */
int  rto_thickness_histogram(rto_context* ctx, int64_t* out, int64_t capacity, int64_t* bins);
/* Device time in ms of the last rto_thickness_field: transform (its three passes), gather, summary (-1: not run). */
int  rto_last_thickness_ms(const rto_context* ctx, float ms[3]);
/* The gather's offset table depends on c alone; the context keeps the one of the last c from call to call, across grids, and
 * builds another only when c changes.  *table_c = the c it was made for (0: none yet), *built = tables built so far (both may be
 * NULL).  No value of any field depends on it. */
int  rto_debug_thickness_table(const rto_context* ctx, int* table_c, int64_t* built);

/* ---- component measures -------------------------------------------------------
 * What every piece of the resident labelling measures: its surface by direction, its first and second moments (centre of mass,
 * principal axes) and its Euler number (blob, ring or shell: pieces - tunnels + cavities).  How much surface a piece that a carve
 * cut loose has, whether a voxelized part has a through-hole.  No reference counterpart.  Every number is an integer sum over a
 * voxel and its 3 x 3 x 3 neighbours that a brute-force loop over rto_download_labels reproduces bit for bit.
 *
 * Rule.  Measures describe the RESIDENT LABELLING: the set (RTO_SET_SOLID / RTO_SET_EMPTY) and the
 * connectivity (RTO_CONN_FACE / RTO_CONN_FULL) of the last rto_label_components.  "In the set" means label >= 0; voxels outside
 * the grid are not in the set; voxel (i, j, k) has linear index v = i + dimX (j + dimY k).  One record per component, in the
 * table's order, and one for the whole set (the total row):
 *   voxels    the component's size (== rto_component.voxels).
 *   faces[d]  the voxels of the component whose neighbour in direction d (-x, +x, -y, +y, -z, +z) is not in the set; a neighbour
 *             beyond the grid is not in the set.  Both connectivities join face neighbours, so a face neighbour that is in the
 *             set is in the same component.
 *   cells     under RTO_CONN_FULL the component is read as a union of closed unit cubes: n0, n1, n2 are the numbers of distinct
 *             lattice vertices, edges and faces incident to at least one of its voxels.  Two voxels that share a vertex are
 *             26-adjacent, so every such cell belongs to exactly one component; it is counted at the incident set voxel with
 *             the smallest linear index.
 *             Under RTO_CONN_FACE: P the face-adjacent pairs with both voxels in the set, Q the axis-aligned 2 x 2 squares with
 *             all four in the set, O the 2 x 2 x 2 blocks with all eight in the set, each counted at its lowest corner.  A fully
 *             set pair, square or block is face-connected, so it lies in one component.
 *   euler     FULL: n0 - n1 + n2 - voxels.  FACE: voxels - P + Q - O.  The component's Euler number under its connectivity:
 *             pieces (1) - tunnels + cavities.
 *   sum       of i, of j, of k over the component's voxels;  sum2 of ii, jj, kk, ij, ik, jk.
 *   total     the sum of the records field by field; cells are disjoint between components, so its euler is the Euler number
 *             of the whole set.  All zero for an empty set.
 * Range: a grid with a dimension above 32768 is RTO_E_UNSUPPORTED; below that every sum stays under 2^61 (voxels <= 2^31, an
 * index is below 2^15).
 * rto_measure_components keeps the table resident beside the labels; it is freed wherever the labels are freed (every call that
 * changes or replaces the grid, a fresh rto_label_components, rto_destroy) and the readers then return RTO_E_INVALID.  The total
 * is made on the device: no download of the table.  Synchronous on the context's stream.
 * Errors, each leaving the context untouched: RTO_E_INVALID (no resident labels; too small a capacity; no resident measures, for
 * the readers); RTO_E_UNSUPPORTED (a dimension above 32768). */
#define RTO_MEASURE_MAX_DIM 32768
typedef struct rto_measure {      /* 160 bytes */
    int64_t voxels;               /* == rto_component.voxels */
    int64_t faces[6];             /* exposed faces by direction: -x, +x, -y, +y, -z, +z */
    int64_t cells[3];             /* FULL: n0, n1, n2   FACE: P, Q, O */
    int64_t euler;                /* FULL: n0 - n1 + n2 - voxels   FACE: voxels - P + Q - O */
    int64_t sum[3];               /* sum of i, of j, of k */
    int64_t sum2[6];              /* sum of ii, jj, kk, ij, ik, jk */
} rto_measure;

int  rto_measure_components(rto_context* ctx, rto_measure* total /* may be NULL */);
/* The resident table: *count records (may be NULL); out == NULL: the count alone. */
int  rto_download_measures(rto_context* ctx, rto_measure* out, int64_t capacity, int64_t* count);
/* The resident table (a device pointer the context owns, valid until the measures are freed). */
int  rto_measures_device(rto_context* ctx, rto_measure** d_measures, int64_t* count);
/* Device time in ms of the last rto_measure_components: the measuring kernels (with the memset in front), the total (-1: not run). */
int  rto_last_measure_ms(const rto_context* ctx, float ms[2]);

/* ---- skeletons: topology-preserving thinning -----------------------------------
 * The centreline of a shape of the resident grid: the one-voxel-wide curve down the middle of a corridor, a duct or a pore, the
 * ring that is left of a part with a through-hole, the centred curve between two doors.  The set is peeled layer by layer, and a
 * voxel leaves only when its going changes neither the pieces nor the tunnels nor the cavities of the set.  No reference
 * counterpart.  Every result is an integer that a plain loop over rto_download_voxels reproduces bit for bit.
 *
 * Rule:
 *   index     voxel (i, j, k) has linear index v = i + dimX (j + dimY k); the sets are rto_label_components': RTO_SET_SOLID the
 *             voxels equal to 1, RTO_SET_EMPTY the voxels equal to 0.  A voxel outside the grid is NOT IN THE SET: this is the
 *             convention of the component measures (section 22), under which their Euler number is the invariant here, and not
 *             that of the distance fields (section 19), where the outside is no set at all.  So a set that touches a face of the
 *             grid is peeled from that face too.
 *   conn      X is the current set.  RTO_CONN_FULL joins X by 26 and its complement by 6; RTO_CONN_FACE joins X by 6 and its
 *             complement by 26.
 *   simple    N26*(p): the 26 neighbours of p; N18*(p): those that differ from p on at most two axes; N6*(p): the face
 *             neighbours.  Under FULL p is simple when X n N26*(p) is non-empty and 26-connected within itself and, with
 *             B = N18*(p) \ X, the set B n N6*(p) is non-empty and lies in one 6-connected component of B.  Under FACE the same
 *             with the roles exchanged: X n N6*(p) is non-empty and lies in one 6-component of X n N18*(p), and N26*(p) \ X is
 *             non-empty and 26-connected; that is simple_FULL of the complemented neighbourhood.
 *   pass      p = 1, 2, ...  Mark: M = the voxels of X with a neighbour not in X (the 6 face neighbours under FULL, the 26 under
 *             FACE), fixed for the whole pass: a pass peels at most one layer.  Then sub-steps s = 0 .. 7 in this order:
 *             subfield s is the voxels with (i & 1) + 2 (j & 1) + 4 (k & 1) == s, and every voxel of subfield s that is in M, is
 *             no anchor, is not kept by the mode and is simple, each read from the current X, leaves X, all of them at once.
 *             Two voxels of one subfield are never 26-adjacent, so removing them together is removing them one after the other
 *             in any order, each a simple point: pieces, tunnels and cavities of X are preserved, and nothing depends on
 *             scheduling.  The first pass that removes nothing ends the thinning; so does max_passes.
 *   modes     RTO_SKEL_TOPOLOGY keeps nothing extra: a blob becomes one voxel, a ring a closed curve, a shell a closed surface.
 *             RTO_SKEL_CURVE keeps a voxel that has exactly one neighbour in X among its 26 (a curve's end); it needs
 *             RTO_CONN_FULL.
 *   anchors   n >= 0 linear indices, on the host, duplicates allowed.  An index outside [0, voxels) is RTO_E_INVALID; an anchor
 *             that is not in the set is ignored; an anchor is never removed.  Two anchors in a simply connected space under
 *             TOPOLOGY leave a centred curve between them.
 *   field     k[v] as int32: -1 for a voxel not in the set, 0 for a voxel that stays (the skeleton), p >= 1 for the pass that
 *             removed it.  A run with max_passes = m leaves exactly {k == 0 or k > m} of the unlimited run.
 *   limit     max_passes below 1 is RTO_E_INVALID; RTO_SKEL_NO_LIMIT or more: none.
 *   summary   kept the voxels with k == 0, removed those with k > 0, passes the largest k (the passes that removed something).
 *   edit      rto_edit_skeleton makes its own field (the resident one is not consulted) and flips every voxel with k > 0: set
 *             SOLID becomes EMPTY (0), set EMPTY becomes FILLED (1).  *changed (may be NULL) = voxels flipped.  When it is > 0
 *             the context is left exactly as rto_edit_voxels leaves it after a change (labels, measures and the distance,
 *             geodesic, thickness and skeleton fields freed); changed == 0 touches nothing.  Idempotent: a second call changes 0.
 * rto_skeleton_field keeps the volume (int32 per voxel) resident beside the other fields, with its set, connectivity and mode;
 * every call that changes or replaces the grid frees it as it frees them, and the readers then return RTO_E_INVALID.
 * Synchronous on the context's stream.
 * Errors, in rto_geodesic_field's order, each leaving the context untouched: RTO_E_INVALID (unknown set, connectivity or mode;
 * CURVE with FACE; n < 0, or NULL anchors with n > 0; max_passes below 1; an anchor out of range; too small a capacity; no resident
 * skeleton field, for the readers); RTO_E_NO_OCTREE (no octree built); RTO_E_UNSUPPORTED (the octree came from rto_upload_octree:
 * no resident grid; more than 2^31 - 2 voxels); RTO_E_INTERNAL (more than voxels + 1 passes: every pass but the last removes a
 * voxel). */
#define RTO_SKEL_TOPOLOGY 0
#define RTO_SKEL_CURVE    1
#define RTO_SKEL_NO_LIMIT 0x7fffffff
typedef struct rto_skel_summary {   /* 32 bytes */
    int64_t kept;                   /* voxels with k == 0: the skeleton */
    int64_t removed;                /* voxels with k > 0 */
    int64_t passes;                 /* the largest k: the passes that removed something */
    int64_t reserved;               /* 0 */
} rto_skel_summary;

int  rto_skeleton_field(rto_context* ctx, int set, int connectivity, int mode, const int64_t* anchors /* may be NULL when n is 0 */,
                        int64_t n, int64_t max_passes, rto_skel_summary* summary /* may be NULL */);
/* dimZ x dimY x dimX int32, x fastest. */
int  rto_download_skeleton(rto_context* ctx, int32_t* out, int64_t capacity);
/* The resident field (a device pointer the context owns, valid until the field is freed). */
int  rto_skeleton_device(rto_context* ctx, int32_t** d_k);
int  rto_edit_skeleton(rto_context* ctx, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t max_passes,
                       int64_t* changed /* may be NULL */);
/* Device time in ms of the last rto_skeleton_field: init, thinning (all passes, with the host's looks at the device), summary
 * (-1: not run). */
int  rto_last_skeleton_ms(const rto_context* ctx, float ms[3]);
/* Device time in ms of the last rto_edit_skeleton: field and flip, octree rebuild, triangle rebuild (-1: not run). */
int  rto_last_skeleton_edit_ms(const rto_context* ctx, float ms[3]);
/* The last rto_skeleton_field: kernel launches of the thinning (one mark and eight sub-steps per pass sent out, the passes behind
 * the fixed point included) and the tiles run summed over the sub-steps (may be NULL). */
int  rto_debug_skeleton_passes(const rto_context* ctx, int64_t* launches, int64_t* tiles_run);
/* How many passes go out between two looks of the host at the device (1 .. 64, 8 by default).  A tuning choice: passes behind the
 * fixed point remove nothing, so no value of any field or edit depends on it. */
int  rto_debug_set_skeleton_look(rto_context* ctx, int passes_per_look);

/* ---- exposure fields: sun hours and sky view per voxel --------------------------
 * Which air voxels see the sun at these hours, how much of the sky does each see, which stay dark: for every evaluated EMPTY voxel
 * the sum of the weights of the directions along which nothing of the grid stands in the way.  Directional and independent of any
 * camera; exact in integers.  No reference counterpart.  Every result is an integer that a plain loop over rto_download_voxels
 * reproduces bit for bit.
 *
 * Rule:
 *   index     voxel p = (i, j, k) has linear index v = i + dimX (j + dimY k); SOLID the voxels equal to 1, EMPTY the voxels equal
 *             to 0.  Voxels outside the grid do not exist: they block nothing, and beyond the grid is open sky.
 *   direction d = (a, b, c), three int32, not all zero, every |component| <= RTO_EXPO_MAX_COMP.  Only the line matters: d and g d
 *             give the same result.
 *   ray       the open half line centre(p) + t d, t > 0.  In doubled integer coordinates the centre is P = 2 p + 1 and voxel q is
 *             the open cube (2 q, 2 q + 2)^3.
 *   crossed   a voxel q != p is crossed when the ray meets q's open cube: there is a t > 0 with P + t d strictly inside on all
 *             three axes.  A ray through an edge or a corner crosses neither of the cubes it only touches: from p, direction
 *             (1, 1, 0) crosses p + (1, 1, 0), but neither p + (1, 0, 0) nor p + (0, 1, 0).
 *   reach     r >= 1, in voxels: only crossed voxels with max-norm |q - p| <= r can block.  RTO_EXPO_NO_LIMIT or more: no limit;
 *             below 1 is RTO_E_INVALID.
 *   blocked   (p, d) is blocked when some crossed voxel inside the grid and within reach is SOLID.
 *   weights   n int32 weights w_d >= 0 (hours, cosine weights of a sky dome, irradiance), or NULL for all ones; their sum W must
 *             be <= 2^31 - 1.  A direction given twice counts twice.
 *   evaluated RTO_EXPO_ALL: every EMPTY voxel.  RTO_EXPO_SKIN: the EMPTY voxels with at least one SOLID voxel among their 6 face
 *             neighbours: the air voxel in front of every exposed face, where a facade's exposure is read.
 *   field     e[v] as int32: for an evaluated voxel the sum of w_d over the directions that are not blocked; -1 for every other.
 *   summary   evaluated; total, the sum of e over the evaluated voxels; dark, those with e == 0; open, those with e == W.  With
 *             nothing evaluated: 0, 0, 0, 0.
 * rto_exposure_field keeps the volume (int32 per voxel) resident beside the other fields, with its n, W, mode and reach; every call
 * that changes or replaces the grid frees it as it frees them, and the readers then return RTO_E_INVALID.  Synchronous on the
 * context's stream.
 * Errors, in rto_geodesic_field's order, each leaving the context untouched: RTO_E_INVALID (NULL dirs; n below 1 or above
 * RTO_EXPO_MAX_DIRS; a zero direction or a component beyond +-255; a negative weight or W above 2^31 - 1; unknown mode; reach below
 * 1; too small a capacity; no resident exposure field, for the readers); RTO_E_NO_OCTREE (no octree built); RTO_E_UNSUPPORTED (the
 * octree came from rto_upload_octree: no resident grid; more than 2^31 - 2 voxels). */
#define RTO_EXPO_ALL      0
#define RTO_EXPO_SKIN     1
#define RTO_EXPO_MAX_COMP 255
#define RTO_EXPO_MAX_DIRS 1024
#define RTO_EXPO_NO_LIMIT 0x7fffffff
typedef struct rto_expo_summary {   /* 32 bytes */
    int64_t evaluated;              /* voxels with e >= 0 */
    int64_t total;                  /* the sum of e over them */
    int64_t dark;                   /* evaluated voxels with e == 0 */
    int64_t open;                   /* evaluated voxels with e == W */
} rto_expo_summary;

int  rto_exposure_field(rto_context* ctx, const int32_t* dirs /* n x 3 */, const int32_t* weights /* n, may be NULL */, int n,
                        int mode, int reach, rto_expo_summary* summary /* may be NULL */);
/* dimZ x dimY x dimX int32, x fastest. */
int  rto_download_exposure(rto_context* ctx, int32_t* out, int64_t capacity);
/* The resident field (a device pointer the context owns, valid until the field is freed). */
int  rto_exposure_device(rto_context* ctx, int32_t** d_e);
/* Device time in ms of the last rto_exposure_field: prepare (bit rows, selection, templates), march, summary (-1: not run). */
int  rto_last_exposure_ms(const rto_context* ctx, float ms[3]);

/* ---- part segmentation: watershed of the distance field, parts and necks ----------
 * Which parts is one component made of?  Two grains that touch, two rooms joined by a door, the pores and throats of one
 * cavity: every voxel of a set climbs to the nearest local maximum of its distance to the surface, and basins whose connecting
 * neck is wide relative to the smaller of the two are merged.  No reference counterpart.  Every result is an integer that a plain
 * loop over rto_download_voxels reproduces bit for bit.
 *
 * Rule.  Index, sets and connectivity are rto_label_components'; voxels outside the grid belong to no set.
 *   height    for v in the set S, h[v] is rto_distance_field's uncapped d2 from v to the voxels of the grid NOT in S (the transform
 *             of the other set): h >= 1 on S, 0 off it; RTO_DIST_NONE on all of S when the grid has no voxel outside S.
 *   order     key(v) = (h[v], -v), compared lexicographically: a strict total order, so plateaus do not exist.
 *   ascent    up(v) is the neighbour of v under the connectivity, inside S, with the largest key, if that key exceeds key(v);
 *             otherwise v is a peak and up(v) = v.  The basin of a peak is every voxel whose up chain ends there.  Basins are
 *             numbered in ascending order of their peak's linear index.
 *   passes    for every pair of adjacent voxels (a, b) of S in different basins the pass height is min(h[a], h[b]) and its index
 *             min(a, b).  A basin edge (A < B by number) holds s, the largest pass height; at, the smallest pass index that
 *             attains it; pairs, the number of such voxel pairs.
 *   merge     ratio is an integer in [0, RTO_PARTS_RATIO_MAX].  Basin edges are processed in the order (s descending, A ascending,
 *             B ascending); a union-find over basins carries P(cluster), the largest peak height in it.  Edge (A, B) joins
 *             find(A) != find(B) exactly when 1,000,000 s >= ratio^2 min(P(find A), P(find B)) in int64; on a join P becomes the
 *             larger of the two.  ratio = 0 joins every adjacent pair: the parts are the components and the label volume equals
 *             rto_label_components' bit for bit.  ratio = 1001 joins nothing: the parts are the basins.  ratio = 1000 joins only
 *             across passes as high as the lower peak (the fragments of a flat top).  No monotonicity in ratio is claimed: merges
 *             raise P and make later tests stricter.
 *   parts     the clusters, numbered in ascending order of their smallest voxel index; the label volume is int32, -1 off S.
 *   necks     one per pair of adjacent parts, sorted by (part_lo, part_hi): h is the largest s among the basin edges between the
 *             two, at is that edge's (ties in s go to the smaller at), pairs is summed.  sqrt(h) voxels is the throat radius.
 *   cut       rto_edit_parts segments afresh (the resident result is not consulted) and flips every voxel v of S that has a
 *             neighbour u in S, under the connectivity, with part[u] > part[v].  Afterwards no two voxels of different parts are
 *             adjacent.  *changed (may be NULL) = voxels flipped; when it is > 0 the context is left exactly as
 *             rto_edit_components leaves it after a change; changed == 0 touches nothing.
 * rto_segment_parts keeps the label volume and both tables resident; they describe the grid they were made from, and every call
 * that changes or replaces the grid frees them (the calls that free the component labels): the readers then return
 * RTO_E_INVALID.  An empty set gives 0 parts, a volume of -1 and empty tables.  Synchronous on the context's stream.
 * Errors, each leaving the context untouched: RTO_E_INVALID (unknown set or connectivity, ratio outside [0, 1001], too small a
 * capacity, nothing resident for the readers); RTO_E_NO_OCTREE; RTO_E_UNSUPPORTED (rto_distance_field's conditions, and a grid of
 * more than 2^31 - 2 voxels); RTO_E_INTERNAL (the ascent did not flatten in 32 rounds, or the basin-edge table was still full after
 * 8 doublings: a defect). */
#define RTO_PARTS_RATIO_MAX 1001
typedef struct rto_part {           /* 64 bytes; the first 48 have rto_component's layout */
    int64_t root;                   /* smallest linear voxel index of the part */
    int64_t voxels;                 /* its size */
    int32_t lo[3], hi[3];           /* inclusive voxel bounding box */
    int32_t touches;                /* as rto_component.touches */
    int32_t basins;                 /* basins merged into the part */
    int64_t peak;                   /* the voxel of the part with the largest key */
    int32_t peak_h;                 /* h there */
    int32_t reserved;               /* 0 */
} rto_part;
typedef struct rto_neck {           /* 32 bytes */
    int32_t part_lo, part_hi;       /* part_lo < part_hi */
    int32_t h;                      /* the highest pass between the two parts */
    int32_t reserved;               /* 0 */
    int64_t at;                     /* the smallest pass index that attains it */
    int64_t pairs;                  /* adjacent voxel pairs between the two parts: the contact area */
} rto_neck;
typedef struct rto_parts_summary {  /* 32 bytes */
    int64_t parts, basins, necks;
    int64_t pairs;                  /* summed over the necks */
} rto_parts_summary;

int  rto_segment_parts(rto_context* ctx, int set, int connectivity, int ratio, rto_parts_summary* summary /* may be NULL */);
/* dimZ x dimY x dimX int32, x fastest. */
int  rto_download_part_labels(rto_context* ctx, int32_t* out, int64_t capacity);
/* out == NULL: the count alone. */
int  rto_download_parts(rto_context* ctx, rto_part* out, int64_t capacity, int64_t* count);
int  rto_download_necks(rto_context* ctx, rto_neck* out, int64_t capacity, int64_t* count);
/* The resident label volume and tables (device pointers the context owns, valid until they are freed); any pointer may be NULL. */
int  rto_parts_device(rto_context* ctx, int32_t** d_labels, rto_part** d_parts, int64_t* parts, rto_neck** d_necks, int64_t* necks);
int  rto_edit_parts(rto_context* ctx, int set, int connectivity, int ratio, int64_t* changed /* may be NULL */);
/* The last rto_segment_parts in ms: the transform, the ascent with its flatten rounds, ranking with the basin table, basin edges
 * (device time each), and the host's merge with the downloads, uploads and the relabel launch (host clock); -1: not run. */
int  rto_last_parts_ms(const rto_context* ctx, float ms[5]);
/* The last rto_segment_parts: basins, basin edges downloaded (one record each), flatten launches up to and including the first
 * that changed nothing, and the slots of the edge table that held them (0: fewer than two basins, no table).  Any may be NULL. */
int  rto_debug_parts(const rto_context* ctx, int64_t* basins, int64_t* edges, int* rounds, int64_t* capacity);
/* The first capacity of the edge table from now on (rounded up to a power of two; 0: sized from the basin count).  A table that
 * fills up is discarded and made again with twice the slots, at most 8 times: no value depends on the capacity. */
int  rto_debug_parts_capacity(rto_context* ctx, int64_t first_capacity);

/* ---- field views ------------------------------------------------------------
 * A frame of the octree, from the renders' camera, coloured by an int32 volume of the resident grid: a resident field, the
 * component labels or a caller's own volume; and per pixel the value under it.  The reference shows per-voxel
 * data with its second renderer (VolumeRaycastRenderer, a GL path); this is the exact-integer form of that need.  All float
 * arithmetic is float32, one IEEE operation per operator, in the order written.  Rule:
 *   ray       the frame's pixel ray (generate_ray_tab: rto_render_device's).  Like the queries, the view ignores rto_update_frustum.
 *   window    without a clip box (0, largest float below 1e30).  With one (clip != 0): the planes of axis a are
 *             gridMin[a] + (float)i * voxelSize for i = clip_lo[a] and clip_hi[a]; t1 = (lo plane - o) * (1 / d), t2 = (hi plane - o) *
 *             (1 / d) per axis, tNear = max(max(min(t1x, t2x), min(t1y, t2y)), min(t1z, t2z)), tFar likewise with min and max
 *             exchanged (glm's min and max, the queries' slab formula); a ray that fails tNear <= tFar && tFar > 0 is a miss;
 *             t_lo = max(0, tNear), t_hi = min(below 1e30, tFar).
 *   hit       the box query of `mode` (RTO_QUERY_FIRST or RTO_QUERY_CLOSEST) in [t_lo, t_hi]: leaf, tHit and face exactly as
 *             rto_query_* define them.  FIRST without a clip box hits the pixels rto_render_device and rto_render_lit_* hit.
 *   voxel     p = o + d * tHit per component.  On every axis c: q = floor((p[c] - gridMin[c]) / voxelSize), clamped (as a float; a
 *             NaN goes to the lower end) into the leaf's [lo, lo + size - 1], converted to int and, with a clip box, clamped into
 *             [clip_lo[c], clip_hi[c] - 1].  Then, when face >= 0, the face's axis a = face >> 1 drops its q and takes the leaf's
 *             own boundary voxel: lo + size - 1 for an odd face, lo for an even one.  Leaves of one voxel are therefore exact
 *             whatever the floats do; larger leaves, and leaves the clip box cuts, follow the float statement.
 *   sample    RTO_SAMPLE_HIT: that voxel.  RTO_SAMPLE_FRONT: that voxel moved by one along the entry face's outward normal (+1 on
 *             axis a for an odd face, -1 for an even one): the EMPTY voxel in front of the surface, where exposure SKIN fields and
 *             distance-to-SOLID fields live.  FRONT has no voxel when face == -1, and none when the neighbour lies outside the
 *             grid's dims.
 *   value     what d_values holds: RTO_FIELD_PIXEL_MISS for a miss; RTO_FIELD_PIXEL_NONE when there is no voxel or the volume's
 *             value there lies outside [valid_lo, valid_hi]; otherwise that value.  The defaults valid_lo = 0 and valid_hi =
 *             0x7ffffffe leave out -1 ("outside the set") and RTO_DIST_NONE.
 *   summary   hits (pixels that are no miss), valued, vmin and vmax over the valued pixels (0 and 0 when there are none), and the
 *             range (lo, hi) the colours used: (range_lo, range_hi), or (vmin, vmax) when range_lo == range_hi (auto range).  It is
 *             made on the device and the colour pass reads it there: no frame has a host step or a synchronisation.
 *   index     of a valued pixel of value v, in int64: w = clamp(v, lo, hi) - lo, s = hi - lo.  CATEGORY: mix32((uint32)v) & 255
 *             with the lit render's mix32, whatever the range.  Otherwise s == 0 gives 0; LINEAR floor(w * 255 / s); SQRT the
 *             largest k in 0..255 with k * k * s <= w * 65025 (squared distances and thicknesses then read linearly).
 *   bins      bins[k] = valued pixels of index k: the legend.  Their sum is `valued`.
 *   colour    a LUT entry is the bytes r, g, b, a in memory order; each channel is (float)byte / 255.0f.  With shade != 0 r, g
 *             and b are each multiplied by (0.25f + 0.75f * ndotl), ndotl = shade_term's Lambert term of the hit leaf against
 *             the renders' light (computed from the leaf's own box: its tHit is max(0, tNear) of that box, also when a clip box
 *             cut the leaf); alpha is untouched.  Miss pixels are miss_rgba, pixels without a value none_rgba, both unshaded.
 * The volume is int32, dimZ x dimY x dimX, x fastest.  RTO_FIELD_DISTANCE .. RTO_FIELD_PARTS are the resident fields
 * (rto_distance_field .. rto_segment_parts), RTO_FIELD_LABELS the component labels, RTO_FIELD_CALLER the caller's
 * volume (for the other sources it must be NULL).  Needs a canonical tree and a resident grid: what rto_build_octree,
 * rto_voxelize_mesh and the edits leave.  A tree that is one leaf is rendered (its box is the walk).  rto_set_kernel does not apply.
 * A whole-grid clip box gives the frame without one when the grid's planes are computed without rounding (both forms of a plane
 * are then the same float).
 * Errors, each leaving the context untouched, checked in this order: RTO_E_INVALID: a NULL frame, view, LUT or rgba; a misaligned
 * buffer (d_rgba 16 bytes, d_summary and d_bins 8, d_lut, d_volume and d_values 4); an unknown source, sample, mode (ANY is
 * invalid) or scale; reserved != 0; valid_lo > valid_hi or valid_lo <= INT32_MIN + 1; range_lo > range_hi; a width or height
 * below 1; a frame beyond the lit render's limits (width * height + 128 and 64 * (8x8 tiles) + 256 below 2^32); CALLER without a
 * volume, or a volume with another source.  RTO_E_NO_OCTREE: nothing uploaded.  RTO_E_UNSUPPORTED: no resident grid
 * (rto_upload_octree), then a non-canonical array.  RTO_E_INVALID: a clip box with clip_lo[a] < 0, clip_hi[a] > dim[a] or
 * clip_lo[a] >= clip_hi[a]; last, a named source that is not resident, in its readers' words ("... not made yet, or the grid has
 * changed since").
 * The device form is asynchronous on hip_stream.  Its work buffers (the summary block, and a value buffer when d_values is NULL)
 * live on the context under the lit render's rules: a frame larger than any before allocates, and then must not be stream-
 * captured; one set per context, so field views on different streams of one context must not run at the same time.  With
 * shade != 0 the first pass parks ndotl in the red channel of d_rgba before the second pass overwrites the pixel. */
#define RTO_FIELD_DISTANCE  0
#define RTO_FIELD_GEODESIC  1
#define RTO_FIELD_THICKNESS 2
#define RTO_FIELD_SKELETON  3
#define RTO_FIELD_EXPOSURE  4
#define RTO_FIELD_PARTS     5
#define RTO_FIELD_LABELS    6
#define RTO_FIELD_CALLER    7
#define RTO_SAMPLE_HIT      0
#define RTO_SAMPLE_FRONT    1
#define RTO_SCALE_LINEAR    0
#define RTO_SCALE_SQRT      1
#define RTO_SCALE_CATEGORY  2
#define RTO_FIELD_PIXEL_MISS (-2147483647 - 1)   /* INT32_MIN */
#define RTO_FIELD_PIXEL_NONE (-2147483647)       /* INT32_MIN + 1 */
typedef struct rto_field_view {     /* 112 bytes */
    int32_t  source;                /* RTO_FIELD_* */
    int32_t  sample;                /* RTO_SAMPLE_* */
    int32_t  mode;                  /* RTO_QUERY_FIRST or RTO_QUERY_CLOSEST */
    int32_t  scale;                 /* RTO_SCALE_* */
    int32_t  valid_lo, valid_hi;    /* values outside are "no value"; defaults 0 and 0x7ffffffe; valid_lo > INT32_MIN + 1 */
    int32_t  range_lo, range_hi;    /* equal: auto range */
    int32_t  clip;                  /* != 0: the section box below applies */
    int32_t  clip_lo[3], clip_hi[3];   /* voxel indices, x y z: 0 <= clip_lo < clip_hi <= dim */
    int32_t  shade;                 /* != 0: colours are multiplied by 0.25 + 0.75 ndotl */
    float    miss_rgba[4];
    float    none_rgba[4];
    int32_t  reserved[4];           /* 0 */
} rto_field_view;
typedef struct rto_field_view_summary {   /* 32 bytes */
    int64_t  hits;                  /* pixels that are no miss */
    int64_t  valued;                /* pixels that hold a value */
    int32_t  vmin, vmax;            /* over the valued pixels; 0, 0 when there are none */
    int32_t  lo, hi;                /* the range the colours used */
} rto_field_view_summary;

int  rto_render_field_device(rto_context* ctx, const rto_frame* frame, const rto_field_view* view, const uint32_t* d_lut /* 256 */,
                             const int32_t* d_volume /* RTO_FIELD_CALLER only */, void* d_rgba /* float4 per pixel, 16-byte aligned */,
                             int32_t* d_values /* may be NULL */, rto_field_view_summary* d_summary /* may be NULL */,
                             int64_t* d_bins /* 256, may be NULL */, void* hip_stream);
/* The same with host buffers (the LUT and a caller's volume too); synchronous on the context's stream. */
int  rto_render_field_host(rto_context* ctx, const rto_frame* frame, const rto_field_view* view, const uint32_t* lut /* 256 */,
                           const int32_t* volume /* RTO_FIELD_CALLER only */, float* host_rgba, int32_t* host_values /* may be NULL */,
                           rto_field_view_summary* host_summary /* may be NULL */, int64_t* host_bins /* 256, may be NULL */);
/* Device time of the last field view's two kernels in ms (sample, shade); waits for that frame.  -1: not run, or the frame was
 * stream-captured or launched after rto_timing_begin(ctx, -1). */
int  rto_last_field_view_ms(const rto_context* ctx, float ms[2]);

/* ---- field projections ------------------------------------------------------
 * A frame from the renders' camera whose pixel value is a reduction of an int32 volume of the resident grid over the voxels the
 * pixel ray crosses in the grid, or in a section box: maximum, minimum, mean, count or the first value inside [valid_lo, valid_hi];
 * coloured as a field view is.  The reference marches its dense volume per pixel in VolumeRaycastRenderer;
 * this is the exact-integer form of that march.  The octree is not walked.  "Valued": a voxel whose value lies in [valid_lo,
 * valid_hi].  All float arithmetic is float32, one IEEE operation per operator, in the order written; the only floats are the plane
 * parameters T below, so floats decide which voxels a ray visits and nothing else.  Rule:
 *   ray       the frame's pixel ray o, d, inv = 1.0f / d (generate_ray_tab: rto_render_device's).  rto_update_frustum is ignored.  A
 *             ray with a non-finite component of o, or with all three axes still, is a miss.
 *   planes    P_a(j) = gridMin[a] + (float)j * voxelSize for j = 0 .. dim[a] (the field views' clip-plane formula), and T_a(j) =
 *             (P_a(j) - o[a]) * inv[a].  Float rounding is monotone, so T_a is non-decreasing in j when inv[a] > 0 and
 *             non-increasing otherwise.
 *   still     axis a is still when inv[a] is not finite (d[a] is 0, -0.0, or so small that 1 / d overflows).  Its coordinate is
 *             floor((o[a] - gridMin[a]) / voxelSize) for the whole ray, and no plane of it is an event.
 *   events    a pair (moving axis a, plane j) with T_a(j) > 0.  Events are ordered by (T, a), x before y before z; events of one
 *             axis with equal T in its direction of travel.  Planes with T_a(j) <= 0 are crossed at the start.
 *   states    the coordinate of a moving axis is crossed - 1 when inv[a] > 0 and dim[a] - crossed otherwise, `crossed` being the
 *             number of its planes crossed so far: it runs from -1 (or dim) outside the grid, through it, to the other outside.
 *             The walk is the start state and then the state after every event, in order.
 *   visited   the states with lo[a] <= c[a] < hi[a] on all three axes, in walk order; [lo, hi) is the clip box, or [0, dim) without
 *             one.  There is no slab test and no t window: a section box filters the whole-grid walk, so boxes that partition the
 *             grid partition every ray's visited voxels, and counts and sums add up exactly.
 *   value     RTO_FIELD_PIXEL_MISS when no voxel is visited; RTO_FIELD_PIXEL_NONE when none of the visited is valued (under
 *             COUNT too); else MAX the largest and MIN the smallest valued value, MEAN floor(sum / count) in int64 towards minus
 *             infinity, COUNT the number of valued voxels, FIRST the value of the first valued voxel in walk order.
 *   voxel     d_voxels: the linear index (z * dimY + y) * dimX + x of the deciding voxel, -1 without one: under MAX and MIN the
 *             first voxel in walk order that holds the pixel's value, under MEAN, COUNT and FIRST the first valued voxel.
 *   totals    d_sums (int64) and d_counts: the sum and the number of the valued voxels visited, under every op; 0 and 0 for a
 *             miss or NONE.
 *   colours   d_rgba, d_summary and d_bins come from the pixel values by the field views' summary, index, bins and colour rules,
 *             unchanged and unshaded: a projection has no surface.
 * The march skips 8 x 8 x 8 bricks through a table of each brick's largest and smallest valued value, rebuilt by every call (it
 * depends on the window, and a caller's volume may have changed).  The table changes no output (rto_debug_set_projection_table).
 * Sources are the field views'.  Needs a resident grid (rto_build_octree, rto_voxelize_mesh, the edits) of fewer than 2^31
 * voxels; the tree need not be canonical.
 * Errors, each leaving the context untouched, checked in this order: RTO_E_INVALID: a NULL frame, projection, LUT or rgba; a
 * misaligned buffer (d_rgba 16 bytes, d_sums, d_summary and d_bins 8, d_lut, d_volume, d_values, d_voxels and d_counts 4); an
 * unknown source, op or scale; reserved != 0; valid_lo > valid_hi or valid_lo <= INT32_MIN + 1; range_lo > range_hi; a width or
 * height below 1; a frame beyond the lit render's limits; CALLER without a volume, or a volume with another source.
 * RTO_E_NO_OCTREE: nothing uploaded.  RTO_E_UNSUPPORTED: no resident grid (rto_upload_octree), then a grid of 2^31 voxels or more.
 * RTO_E_INVALID: a clip box with clip_lo[a] < 0, clip_hi[a] > dim[a] or clip_lo[a] >= clip_hi[a]; last, a named source that is not
 * resident, in its readers' words.
 * The device form is asynchronous on hip_stream.  Its work buffers (the brick table, the field views' summary block and, when
 * d_values is NULL, their value buffer) live on the context under the field views' rules: a larger grid or frame than any before
 * allocates, and then must not be stream-captured; one set per context, so projections and field views on different streams of
 * one context must not run at the same time. */
#define RTO_PROJECT_MAX    0
#define RTO_PROJECT_MIN    1
#define RTO_PROJECT_MEAN   2
#define RTO_PROJECT_COUNT  3
#define RTO_PROJECT_FIRST  4
typedef struct rto_field_projection {   /* 112 bytes */
    int32_t  source;                /* RTO_FIELD_* */
    int32_t  op;                    /* RTO_PROJECT_* */
    int32_t  scale;                 /* RTO_SCALE_* */
    int32_t  valid_lo, valid_hi;    /* the window of valued voxels; defaults 0 and 0x7ffffffe; valid_lo > INT32_MIN + 1 */
    int32_t  range_lo, range_hi;    /* equal: auto range */
    int32_t  clip;                  /* != 0: the section box below applies */
    int32_t  clip_lo[3], clip_hi[3];   /* voxel indices, x y z: 0 <= clip_lo < clip_hi <= dim */
    float    miss_rgba[4];
    float    none_rgba[4];
    int32_t  reserved[6];           /* 0 */
} rto_field_projection;

int  rto_project_field_device(rto_context* ctx, const rto_frame* frame, const rto_field_projection* projection,
                              const uint32_t* d_lut /* 256 */, const int32_t* d_volume /* RTO_FIELD_CALLER only */,
                              void* d_rgba /* float4 per pixel, 16-byte aligned */, int32_t* d_values /* may be NULL */,
                              int32_t* d_voxels /* may be NULL */, int64_t* d_sums /* may be NULL */, int32_t* d_counts /* may be NULL */,
                              rto_field_view_summary* d_summary /* may be NULL */, int64_t* d_bins /* 256, may be NULL */,
                              void* hip_stream);
/* The same with host buffers (the LUT and a caller's volume too); synchronous on the context's stream. */
int  rto_project_field_host(rto_context* ctx, const rto_frame* frame, const rto_field_projection* projection, const uint32_t* lut /* 256 */,
                            const int32_t* volume /* RTO_FIELD_CALLER only */, float* host_rgba, int32_t* host_values /* may be NULL */,
                            int32_t* host_voxels /* may be NULL */, int64_t* host_sums /* may be NULL */,
                            int32_t* host_counts /* may be NULL */, rto_field_view_summary* host_summary /* may be NULL */,
                            int64_t* host_bins /* 256, may be NULL */);
/* Device time of the last projection's three kernels in ms (bricks, march, shade); waits for that frame.  -1: not run, or the
 * frame was stream-captured or launched after rto_timing_begin(ctx, -1).  Without the table the first is the empty interval. */
int  rto_last_projection_ms(const rto_context* ctx, float ms[3]);
/* Developer aid in the style of RTO_KERNEL_GENERIC: 0 = the march consults no brick table (and none is built), 1 = it does
 * (default).  The same loop runs either way and no output depends on it: for A/B timing and for the test that says so.  The
 * tables of rto_composite_field_* follow the same switch. */
int  rto_debug_set_projection_table(rto_context* ctx, int enabled);

/* ---- field compositing ------------------------------------------------------
 * A frame from the renders' camera in which an int32 volume of the resident grid is seen through: every valued voxel a pixel ray
 * crosses takes colour and opacity from a LUT entry, the entries are composited front to back, and the march can be stopped by
 * the grid's solids.  This is the reference's VolumeRaycastRenderer -- a transfer function, front-to-back
 * alpha compositing, termination -- in exact integers.  The octree is not walked.  Floats decide which voxels are visited and, at
 * the very end, the output colour; everything in between is unsigned 32-bit integers.  All float arithmetic is float32, one IEEE
 * operation per operator, in the order written.  Rule:
 *   ray, planes, still, events, states, visited
 *             the field projections', word for word; [lo, hi) is the clip box, or the grid without one.  rto_update_frustum is
 *             ignored.
 *   valued    a voxel whose value lies in [valid_lo, valid_hi].
 *   index     the field views' index of the value v of a valued voxel under `scale` and the range (range_lo, range_hi), which
 *             must be given: a composite has no auto range (every voxel's colour depends on it, so it has to be known before the
 *             march).  LINEAR and SQRT need range_lo < range_hi; CATEGORY ignores the range.
 *   entry     the LUT entry at that index is the bytes r, g, b, a in memory order; a' = a + (a >> 7) is 0 .. 256 (a byte of 255 is
 *             fully opaque).  A voxel contributes when it is valued and a' != 0.
 *   composite the state is T = 65536 (the transmittance, Q16), R = G = B = 0, count = 0.  For every contributing voxel in walk
 *             order: c = (T * a') >> 8; R += c * r; G += c * g; B += c * b; T -= c; count += 1.  T * a' <= 2^24, and R, G and B
 *             are at most 65536 * 255 = 16,711,680 < 2^24: their conversion to float32 is exact.
 *   end       the walk ends at whichever comes first.  Occluded: with occlude != 0, at the first visited voxel whose byte in the
 *             resident grid is 1 (FILLED), before that voxel can contribute.  Saturated: after the first contribution that leaves
 *             T <= stop_q16 (0 .. 65535; with 0 the walk ends only when nothing more can be seen).  Through: when the visited voxels
 *             run out.
 *   outputs   d_transmittance (uint32): T, 65536 for a miss (a ray that visits no voxel).  d_first: the linear index (z * dimY +
 *             y) * dimX + x of the first contributing voxel, -1 without one.  d_stops: the occluding or the saturating voxel, -1
 *             when the walk went through or missed.  d_counts: the contributions.  Each may be NULL.
 *   colour    bg is d_under[pix] (a float4 per pixel) when d_under is given, and the four formulas below then hold for every pixel,
 *             a miss with its T = 65536 and R = G = B = 0 included.  d_under may be d_rgba itself: each pixel is read and then
 *             written by its own lane.  Without d_under, bg is background_rgba for a pixel that visits a voxel, and a miss is
 *             miss_rgba, unblended.  tf = (float)T / 65536.0f; out.r = (float)R / 16711680.0f + tf * bg.r, likewise g and b;
 *             out.a = (float)(65536 - T) / 65536.0f + tf * bg.a.
 *   summary   rto_composite_summary: the pixels that visit a voxel, that have a contribution, and whose walk ended saturated or
 *             occluded.  It is made on the device, with no host step.
 * With an all-opaque LUT (every a = 255) a pixel's colour is therefore the LUT colour of its first valued voxel, bit for bit the
 * colour rto_project_field_* gives it under RTO_PROJECT_FIRST (65536 r / 16711680 and r / 255 are the same real number, both
 * divisions round correctly, and T = 0 adds 0 * bg).  With a LUT whose alpha is nowhere 0 and never 255, stop_q16 = 0 and no
 * occlusion, d_counts and d_first are the projections' d_counts and FIRST's d_voxels.
 * The march skips 8 x 8 x 8 bricks through the projections' table of each brick's largest and smallest valued value (a brick with
 * no valued voxel, or, under LINEAR and SQRT, with no LUT entry of a' != 0 between the indices of those two values) and, with
 * occlude, a second table that says whether a brick holds a FILLED voxel; both are rebuilt by every call.  They change no output:
 * rto_debug_set_projection_table(ctx, 0) switches off every table the composite consults too.
 * Sources are the field views'.  Needs a resident grid of fewer than 2^31 voxels; the tree need not be canonical.
 * Errors, each leaving the context untouched, checked in this order: RTO_E_INVALID: a NULL frame, composite, LUT or rgba; a
 * misaligned buffer (d_under and d_rgba 16 bytes, d_summary 8, d_lut, d_volume, d_transmittance, d_first, d_stops and d_counts
 * 4); an unknown source or scale; reserved != 0; valid_lo > valid_hi or valid_lo <= INT32_MIN + 1; LINEAR or SQRT with range_lo
 * >= range_hi; stop_q16 outside 0 .. 65535; occlude other than 0 or 1; a width or height below 1; a frame beyond the lit render's
 * limits; CALLER without a volume, or a volume with another source.  RTO_E_NO_OCTREE: nothing uploaded.  RTO_E_UNSUPPORTED: no
 * resident grid (rto_upload_octree), then a grid of 2^31 voxels or more.  RTO_E_INVALID: a clip box with clip_lo[a] < 0,
 * clip_hi[a] > dim[a] or clip_lo[a] >= clip_hi[a]; last, a named source that is not resident, in its readers' words.
 * The device form is asynchronous on hip_stream.  Its work buffers (the projections' brick table, the solid table and the summary
 * block) live on the context under the field views' rules: a larger grid than any before allocates, and then must not be stream-
 * captured; one set per context, so composites, projections and field views on different streams of one context must not run at
 * the same time. */
typedef struct rto_field_composite {    /* 112 bytes */
    int32_t  source;                /* RTO_FIELD_* */
    int32_t  scale;                 /* RTO_SCALE_* */
    int32_t  valid_lo, valid_hi;    /* the window of valued voxels; defaults 0 and 0x7ffffffe; valid_lo > INT32_MIN + 1 */
    int32_t  range_lo, range_hi;    /* LINEAR and SQRT: range_lo < range_hi; there is no auto range */
    int32_t  clip;                  /* != 0: the section box below applies */
    int32_t  clip_lo[3], clip_hi[3];   /* voxel indices, x y z: 0 <= clip_lo < clip_hi <= dim */
    int32_t  stop_q16;              /* 0 .. 65535: the walk ends once T <= stop_q16 */
    int32_t  occlude;               /* 1: the walk ends at the first FILLED voxel; 0: the volume is seen through the solids */
    float    background_rgba[4];    /* under a pixel that visits a voxel, when d_under is NULL */
    float    miss_rgba[4];          /* a pixel that visits none, when d_under is NULL */
    int32_t  reserved[5];           /* 0 */
} rto_field_composite;
typedef struct rto_composite_summary {  /* 32 bytes */
    int64_t  visited;               /* pixels that visit a voxel */
    int64_t  contributing;          /* pixels with at least one contribution */
    int64_t  saturated;             /* pixels whose walk ended with T <= stop_q16 */
    int64_t  occluded;              /* pixels whose walk ended at a FILLED voxel */
} rto_composite_summary;

int  rto_composite_field_device(rto_context* ctx, const rto_frame* frame, const rto_field_composite* composite,
                                const uint32_t* d_lut /* 256 */, const int32_t* d_volume /* RTO_FIELD_CALLER only */,
                                const void* d_under /* float4 per pixel, 16-byte aligned; may be NULL, may be d_rgba */,
                                void* d_rgba /* float4 per pixel, 16-byte aligned */, uint32_t* d_transmittance /* may be NULL */,
                                int32_t* d_first /* may be NULL */, int32_t* d_stops /* may be NULL */, int32_t* d_counts /* may be NULL */,
                                rto_composite_summary* d_summary /* may be NULL */, void* hip_stream);
/* The same with host buffers (the LUT and a caller's volume too); synchronous on the context's stream.  host_under may be
 * host_rgba. */
int  rto_composite_field_host(rto_context* ctx, const rto_frame* frame, const rto_field_composite* composite, const uint32_t* lut /* 256 */,
                              const int32_t* volume /* RTO_FIELD_CALLER only */, const float* host_under /* may be NULL */,
                              float* host_rgba, uint32_t* host_transmittance /* may be NULL */, int32_t* host_first /* may be NULL */,
                              int32_t* host_stops /* may be NULL */, int32_t* host_counts /* may be NULL */,
                              rto_composite_summary* host_summary /* may be NULL */);
/* Device time of the last composite in ms (the tables, the march, the summary's fold); waits for that frame.  -1: not run, or the
 * frame was stream-captured or launched after rto_timing_begin(ctx, -1).  Without tables, or without d_summary, the interval is
 * empty. */
int  rto_last_composite_ms(const rto_context* ctx, float ms[3]);

/* ---- field isosurfaces ------------------------------------------------------
 * Marching cubes of an int32 volume of the resident grid at a float level, made on the GPU: the offset
 * surface of a distance field, the boundary of "thinner than three voxels", the reach limit of a geodesic flood, as the same
 * 12-float records rto_extract_mesh gives.  This is the reference's marchingCubesVolume (S/MarchingCubes.cpp:622-689) over the
 * voxel centres, its marchingCubesCell / vertexInterp (:544-620) word for word.  All floats are float32, one IEEE operation per
 * operator, in the order written, with no contraction.  rto_update_frustum is ignored.  Rule:
 *   samples   one per voxel, at the voxel centre: origin[a] = gridMin[a] + 0.5f * voxelSize, P_a(i) = origin[a] + (float)i *
 *             voxelSize (the reference's origin + vec3(x, y, z) * spacing with spacing = voxelSize).  i may be -1 or dim under pad.
 *   value     a voxel inside the box [lo, hi) whose volume value v lies in [valid_lo, valid_hi] has the value (float)v; every other
 *             sample -- an unvalued voxel, a voxel outside the box, the pad ring -- takes the float `outside`.  The box is the clip
 *             box, or [0, dim) without one.  The defaults valid = (0, 0x7ffffffe) leave out -1 and RTO_DIST_NONE, as the views do.
 *             Values above 2^24 round to nearest: that is part of the rule.
 *   cells     without pad: cell (x, y, z) for lo[a] <= c < hi[a] - 1 on every axis.  With pad != 0: lo[a] - 1 <= c < hi[a], so a
 *             ring of `outside` samples closes the surface at the box's faces.  A box of one sample along an axis has no cells
 *             without pad: an empty list, not an error.
 *   cell      corners 0..7 at (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1); bit i of the case is set when val_i <
 *             level; the 12 edges join the reference's corner pairs; a vertex is p1 when fabsf(level - v1) < 1e-6f, else p2 when
 *             fabsf(level - v2) < 1e-6f, else p1 when fabsf(v1 - v2) < 1e-6f, else p1 + ((level - v1) / (v2 - v1)) * (p2 - p1) per
 *             component; the triangles are those of the case's triTable row, in row order (the leaf-triangle build's table).
 *   normal    the reference writes a placeholder (0, 1, 0); this writes the face normal by localMC's formula: n = cross(v1 - v0,
 *             v2 - v0), l2 = dot(n, n); when l2 > 0 and finite the normal is n * inversesqrt(l2), otherwise (+0, +0, +0): the
 *             triangle stays in the list and counts as degenerate.  Snapped vertices make degenerate triangles whenever level
 *             equals a sample value: use half-integer levels.
 *   order     cells in the reference's loop order, z slowest, then y, then x; within a cell the table's.
 *   record    12 floats per triangle: v0, v1, v2, normal (rto_extract_mesh's layout).  tri_cell[j] = ((z + 1) * (dimY + 1) + (y + 1))
 *             * (dimX + 1) + (x + 1) of the owning cell, whatever the pad or clip.
 * Both extraction calls are synchronous on the context's stream (one count is read back).  The result is a snapshot in a buffer of
 * its own -- not rto_extract_mesh's: both stay downloadable side by side -- valid until the next isosurface extraction or
 * rto_destroy, untouched by later edits or builds.  An empty result is RTO_OK with 0 triangles.  The refusals below leave the previous
 * isosurface alone; a device failure (RTO_E_HIP) after the output buffer has been replaced by a larger one leaves none.
 * The count pass skips tiles the level does not cross through a table of each 8 x 8 x 8 brick's smallest and largest substituted
 * value, rebuilt by every call; it changes no output, and rto_debug_set_projection_table(ctx, 0) switches it off too.
 * Sources are the field views'.  Errors, each leaving the previous isosurface and the context untouched, checked in this order:
 * RTO_E_INVALID: NULL params; a misaligned volume (4 bytes); an unknown source; reserved != 0; valid_lo > valid_hi or valid_lo <=
 * INT32_MIN + 1; a level or outside that is not finite; pad other than 0 or 1; CALLER without a volume, or a volume with another
 * source.  RTO_E_NO_OCTREE: nothing uploaded.  RTO_E_UNSUPPORTED: no resident grid (rto_upload_octree), then (dimX + 1)(dimY + 1)
 * (dimZ + 1) >= 2^31.  RTO_E_INVALID: a clip box with clip_lo[a] < 0, clip_hi[a] > dim[a] or clip_lo[a] >= clip_hi[a]; last, a
 * named source that is not resident, in its readers' words.  RTO_E_UNSUPPORTED: more than 2^31 - 1 triangles (the count saturates). */
typedef struct rto_iso_params {     /* 64 bytes */
    int32_t  source;                /* RTO_FIELD_* */
    int32_t  valid_lo, valid_hi;    /* the window of valued voxels; defaults 0 and 0x7ffffffe; valid_lo > INT32_MIN + 1 */
    float    level, outside;        /* finite */
    int32_t  pad;                   /* 0 or 1 */
    int32_t  clip;                  /* != 0: the box below applies */
    int32_t  clip_lo[3], clip_hi[3];   /* voxel indices, x y z: 0 <= clip_lo < clip_hi <= dim */
    int32_t  reserved[3];           /* 0 */
} rto_iso_params;
typedef struct rto_iso_summary {    /* 32 bytes */
    int64_t  triangles;
    int64_t  active_cells;          /* cells with at least one triangle */
    int64_t  degenerate;            /* triangles whose normal is (0, 0, 0) */
    int64_t  reserved;
} rto_iso_summary;

int  rto_extract_isosurface_device(rto_context* ctx, const rto_iso_params* params, const int32_t* d_volume /* RTO_FIELD_CALLER only */,
                                   rto_iso_summary* summary /* host; may be NULL */);
/* The same with a caller's volume in host memory. */
int  rto_extract_isosurface_host(rto_context* ctx, const rto_iso_params* params, const int32_t* volume /* RTO_FIELD_CALLER only */,
                                 rto_iso_summary* summary /* may be NULL */);
/* The last isosurface where it lies: num_tris records of 48 bytes and as many int32 (both may be NULL for the count alone). */
int  rto_isosurface_device(rto_context* ctx, void** d_tris, int32_t** d_tri_cell, int64_t* num_tris);
/* Copies it out; tris == NULL and tri_cell == NULL: the count alone.  RTO_E_INVALID: none extracted yet, capacity too small. */
int  rto_download_isosurface(rto_context* ctx, float* tris, int64_t capacity, int32_t* tri_cell /* may be NULL */, int64_t* num_tris);
/* Device time in ms of the last extraction: count (with the brick table), rank, emit (-1: not run, or the box had no cell and no
 * kernel ran).  The read-back of the count and the growth of the output buffer lie between the last two and are in none of them. */
int  rto_last_isosurface_ms(const rto_context* ctx, float ms[3]);

/* ---- dose fields: point sources seen through the grid, per voxel ----------------
 * Which air voxels see these lamps, cameras, antennas or radiation points, how much of each reaches a voxel through how many walls,
 * how much of the street space does the set cover: for every evaluated EMPTY voxel the sum over the sources of the source's weight,
 * attenuated by the number of SOLID voxels the straight segment to the source crosses and, if asked for, by the squared distance.
 * The purpose of the reference's radiation splat, which DESIGN.md section 9 leaves out because the splat ignores the buildings.
 * Exact in integers; every result is an integer that a plain loop over rto_download_voxels reproduces bit for bit.
 *
 * Rule.  Index, layout, SOLID and EMPTY are rto_exposure_field's; the crossing rule is its rule cut to a
 * segment.
 *   source    s = (i, j, k, w), four int32: a voxel of the resident grid and a weight w >= 0.  n sources, 1 <= n <=
 *             RTO_DOSE_MAX_SOURCES; the sum W of the weights must be <= 2^31 - 1.  A source may sit in a SOLID voxel (a lamp on a
 *             wall); a source given twice counts twice.  Both ends of every segment lie in the grid, which is convex: nothing
 *             outside the grid is ever visited.
 *   segment   for an evaluated voxel p and a source s, d = s - p: centre(p) + t d, 0 < t < 1.  A voxel q outside {p, s} is crossed
 *             when some t in (0, 1) puts the point strictly inside q's open cube; on an axis where d is zero q has p's coordinate.
 *             A segment through an edge or a corner crosses neither cube it only touches.  Equivalently: q is crossed by
 *             rto_exposure_field's ray (p, d) and by the ray (s, -d); or: q is an entry of periods 0 .. g - 1 of the template of
 *             d / g, g the gcd of d's components, without the last entry, which is s.
 *   reach     1 <= r <= RTO_DOSE_MAX_REACH, in voxels; RTO_DOSE_NO_LIMIT, and every value above RTO_DOSE_MAX_REACH, means
 *             RTO_DOSE_MAX_REACH; below 1 is RTO_E_INVALID.  A pair whose max-norm |d| exceeds r is out of reach: it contributes
 *             nothing and is not seen.  (1,023 keeps the crossing times on one common denominator in 32 bits; grids with a longer
 *             side are accepted, their far pairs are out of reach.)
 *   walls     k(p, s): the number of crossed voxels that are SOLID.
 *   transmit  a table T[0 .. m - 1] of uint32 in Q16 (65,536 is 1.0), every entry <= 65,536, 1 <= m <= RTO_DOSE_MAX_TABLE; a
 *             pair with k >= m transmits 0.  NULL stands for {65536}: plain line of sight.  T need not be monotone.
 *   falloff   RTO_DOSE_FALLOFF_NONE: D = 1.  RTO_DOSE_FALLOFF_INVERSE_SQUARE: D = max(1, |d|^2), the squared Euclidean length in
 *             voxels.
 *   c(p, s)   floor(((uint64) w T[k] >> 16) / D) for a pair in reach, else 0.  Every c is at most w: no sum leaves int32.
 *   evaluated RTO_DOSE_ALL: every EMPTY voxel.  RTO_DOSE_SKIN: the EMPTY voxels with a SOLID face neighbour (rto_exposure_field's
 *             two sets, with the same values).
 *   field     e[v] as int32: for an evaluated voxel the sum of c(p, s) over the sources; -1 for every other voxel.
 *   coverage  covered[s], one int64 per source: the evaluated voxels in reach of s with k = 0 (p = s counts when p is evaluated).
 *   summary   evaluated; total, the sum of e; dark, the voxels with e == 0; seen, the evaluated voxels with at least one source in
 *             reach and k = 0; peak, the maximum of e; peak_voxel, the smallest linear index that attains it.  With nothing
 *             evaluated: 0, 0, 0, 0, -1, -1.
 * rto_dose_field keeps the volume (int32 per voxel) and the coverage table resident beside the other fields, with its n, W, m,
 * falloff, mode and reach; every call that changes or replaces the grid frees both, and the readers then return RTO_E_INVALID.
 * Synchronous on the context's stream.
 * There is NO RTO_FIELD_* source code for the dose field: the views, projections, composites and isosurfaces show it as
 * rto_dose_device's pointer with RTO_FIELD_CALLER, like any int32 device volume of the caller's.
 * Errors, in this order, each leaving the context and every resident product untouched: RTO_E_INVALID (NULL sources; n below 1 or
 * above RTO_DOSE_MAX_SOURCES; a negative weight or W above 2^31 - 1; m below 1 or above RTO_DOSE_MAX_TABLE; a table entry above
 * 65,536; unknown falloff or mode; reach below 1); RTO_E_NO_OCTREE (no octree built); RTO_E_UNSUPPORTED (the octree came from
 * rto_upload_octree: no resident grid; more than 2^31 - 2 voxels); RTO_E_INVALID (a source outside the grid: the message names the
 * first such source's index).  The readers: RTO_E_INVALID without a resident dose field or with too small a capacity. */
#define RTO_DOSE_ALL                    0
#define RTO_DOSE_SKIN                   1
#define RTO_DOSE_FALLOFF_NONE           0
#define RTO_DOSE_FALLOFF_INVERSE_SQUARE 1
#define RTO_DOSE_MAX_SOURCES            1024
#define RTO_DOSE_MAX_REACH              1023
#define RTO_DOSE_MAX_TABLE              64
#define RTO_DOSE_NO_LIMIT               0x7fffffff
typedef struct rto_dose_summary {   /* 48 bytes */
    int64_t evaluated;              /* voxels with e >= 0 */
    int64_t total;                  /* the sum of e over them */
    int64_t dark;                   /* evaluated voxels with e == 0 */
    int64_t seen;                   /* evaluated voxels with a source in reach and no SOLID voxel crossed on the way */
    int64_t peak;                   /* the maximum of e; -1: nothing evaluated */
    int64_t peak_voxel;             /* the smallest linear index with e == peak; -1: nothing evaluated */
} rto_dose_summary;

int  rto_dose_field(rto_context* ctx, const int32_t* sources /* n x 4: i, j, k, w */, int n,
                    const uint32_t* transmit /* m, NULL: {65536} */, int m,
                    int falloff, int mode, int reach, rto_dose_summary* summary /* may be NULL */);
/* dimZ x dimY x dimX int32, x fastest. */
int  rto_download_dose(rto_context* ctx, int32_t* out, int64_t capacity);
/* The resident field (a device pointer the context owns, valid until the field is freed): the volume to hand to
 * rto_render_field_* / rto_project_field_* / rto_composite_field_* / rto_extract_isosurface_* with RTO_FIELD_CALLER. */
int  rto_dose_device(rto_context* ctx, int32_t** d_e);
/* covered[0 .. n - 1] of the resident field's n sources (capacity: int64 entries, at least n). */
int  rto_download_dose_coverage(rto_context* ctx, int64_t* out /* n */, int64_t capacity);
/* Device time in ms of the last rto_dose_field: prepare (bit rows, selection, uploads), march, summary (-1: not run). */
int  rto_last_dose_ms(const rto_context* ctx, float ms[3]);

/* ---- dual contouring -----------------------------------------------------------
 * The reference's second surface extractor over the resident grid, made on the GPU: one vertex per voxel,
 * placed by the Hermite data of the sign changes around it, and a quad of two triangles wherever a cell and its +X, +Y or +Z
 * neighbour differ -- the same 12-float records rto_extract_mesh and rto_extract_isosurface_* give.  This is the reference's
 * deterministic pair: the per-voxel vertex rule gatherHermiteData(grid, x, y, z, 1) -> calculateIntersection -> generateDualVertex
 * with QEFSolver (S/AdaptiveDualContouringRenderer.cpp:49-161, 1090-1357) and its triangulation buildTrianglesCPU (:377-486), word
 * for word, oddities included.  The adaptive createTriangles path and the shipped GLSL are not.  All floats are float32, one IEEE
 * operation per operator, in the order written, with no contraction; comparisons the reference makes against a double literal
 * (1e-6, 1e-10) are made in double.  rto_update_frustum is ignored.  A voxel is solid when it is FILLED.  Rule:
 *   vertex    of voxel (x, y, z): centre[a] = (gridMin[a] + (float)c[a] * voxelSize) + 0.5f * voxelSize.  Hermite points: for the
 *             voxels x .. min(x + 1, dimX - 1) (likewise y, z; z slowest), for each its +X, +Y, +Z neighbour in that order (skipped
 *             outside the grid), one point per sign change: position p1 + 0.5f * (p2 - p1) with p = gridMin + (float)c * voxelSize;
 *             normal: the central differences of the +-1 scalar (solid: -1; out of grid: +1) on the two axes perpendicular to the
 *             edge, taken at the first voxel, normalised (v * (1.0f / sqrt(dot(v, v)))), or the edge direction when their squared
 *             length is below 1e-10; negated when (dot(normal, edge) > 0) == (the neighbour is solid).  No point: the vertex is the
 *             centre.  Otherwise generateDualVertex(points, centre, voxelSize) in full: bounds centre -+ 0.5f * voxelSize inset by
 *             0.001f * voxelSize; the mass point; the summed normal, when longer than 0.0001f normalised and, with a component
 *             above 0.85f, snapped to that axis: the points whose normalised normal has dot > 0.7f with it give a plane point, the
 *             centre is projected onto that plane and clamped; otherwise QEFSolver: AtA and Atb of the renormalised normals, the
 *             mass point for at most 2 points, else (AtA + 0.3 I)^-1 Atb by glm 0.9.9.7's determinant and inverse, relaxed by 0.7
 *             towards it from the mass point, accepted when its squared distance to the mass point is below the inset cell size
 *             squared and then mixed 0.2 with the mass point (mix(x, y, a) = x * (1 - a) + y * a), else the mass point; clamped;
 *             mixed 0.1 with the mass point.
 *   cells     (x, y, z) with 0 <= c[a] < dim[a] - 1, or, with a clip box, clip_lo[a] <= c[a] < min(clip_hi[a], dim[a] - 1); z slowest.
 *             Vertices are always those of the whole grid: boxes that partition the cells partition the list.  A grid with a
 *             dimension of 1 has no cell: an empty list, not an error.  There is no pad ring: like the reference's loop, the call
 *             does not close the surface at the grid's faces.
 *   faces     each cell tests +X, +Y, +Z in that order; a face exists when solid(c) != solid(c + e_a).  Its four voxels V00, V01,
 *             V11, V10 are c + (0, +y, +x+y, +x) for X, (0, +x, +x+y, +y) for Y, (0, +y, +y+z, +z) for Z; its triangles are
 *             (V00, V01, V11) then (V00, V11, V10) of their vertices.
 *   normal    n = cross(v1 - v0, v2 - v0), l2 = dot(n, n); l2 > 0 and finite: n * (1.0f / sqrt(l2)), negated when the cell's own
 *             voxel is solid; otherwise (+0, +0, +0) and the triangle counts as degenerate.
 *   area rule RTO_DC_AREA_REFERENCE keeps a triangle when 0.5f * sqrt(l2) > 1e-6 (the reference's absolute test: at voxel sizes
 *             near 1 / 512 it drops real triangles); RTO_DC_AREA_NONE keeps every triangle.
 *   record    12 floats per triangle: v0, v1, v2, normal.  tri_cell[j] = (z * dimY + y) * dimX + x of the owning cell.
 *   summary   faces found; triangles kept; triangles dropped by the area rule (kept + dropped = 2 * faces); degenerate triangles
 *             among the kept; vertex_voxels: the voxels that are one of the four of at least one face found and have at least one
 *             Hermite point.
 * rto_extract_dual_contour is synchronous on the context's stream (one count is read back).  The result is a snapshot in a buffer of
 * its own, beside rto_extract_mesh's and the isosurface's, valid until the next dual-contour extraction or rto_destroy, untouched by
 * later edits or builds.  An empty result is RTO_OK with 0 triangles; a box without a cell runs no kernel.  Errors, each leaving the
 * previous list and the context untouched, checked in this order: RTO_E_INVALID: NULL params, an unknown area_rule, reserved != 0.
 * RTO_E_NO_OCTREE: nothing uploaded.  RTO_E_UNSUPPORTED: no resident grid (rto_upload_octree), then more than 2^31 - 1 voxels.
 * RTO_E_INVALID: a clip box with clip_lo[a] < 0, clip_hi[a] > dim[a] or clip_lo[a] >= clip_hi[a].  RTO_E_UNSUPPORTED: more than
 * 2^31 - 1 triangles (the count saturates).  A device failure (RTO_E_HIP) after the output buffer has been replaced by a larger one
 * leaves no list. */
#define RTO_DC_AREA_REFERENCE 0
#define RTO_DC_AREA_NONE      1
typedef struct rto_dc_params {      /* 48 bytes */
    int32_t  area_rule;             /* RTO_DC_AREA_* */
    int32_t  clip;                  /* != 0: the box of cells below applies */
    int32_t  clip_lo[3], clip_hi[3];   /* cell indices, x y z: 0 <= clip_lo < clip_hi <= dim */
    int32_t  reserved[4];           /* 0 */
} rto_dc_params;
typedef struct rto_dc_summary {     /* 48 bytes */
    int64_t  faces;
    int64_t  triangles;             /* kept: the length of the list */
    int64_t  dropped;               /* by the area rule */
    int64_t  degenerate;            /* kept triangles whose normal is (0, 0, 0) */
    int64_t  vertex_voxels;         /* voxels read by a face that have at least one Hermite point */
    int64_t  reserved;
} rto_dc_summary;
typedef struct rto_dual_vertex {    /* 16 bytes */
    float    p[3];
    int32_t  points;                /* Hermite points gathered; -1: the index lies outside the grid (p is 0) */
} rto_dual_vertex;

int  rto_extract_dual_contour(rto_context* ctx, const rto_dc_params* params, rto_dc_summary* summary /* host; may be NULL */);
/* The last list where it lies: num_tris records of 48 bytes and as many int32 (both may be NULL for the count alone). */
int  rto_dual_contour_device(rto_context* ctx, void** d_tris, int32_t** d_tri_cell, int64_t* num_tris);
/* Copies it out; tris == NULL and tri_cell == NULL: the count alone.  RTO_E_INVALID: none extracted yet, capacity too small. */
int  rto_download_dual_contour(rto_context* ctx, float* tris, int64_t capacity, int32_t* tri_cell /* may be NULL */, int64_t* num_tris);
/* Device time in ms of the last extraction: count, rank, emit (-1: not run, or the box had no cell and no kernel ran). */
int  rto_last_dual_contour_ms(const rto_context* ctx, float ms[3]);
/* The vertex of any voxel of the resident grid, one thread per voxel: voxels[i] = (z * dimY + y) * dimX + x; an index outside
 * [0, dimX dimY dimZ) gives points = -1 and zeros.  Synchronous on the context's stream.  Errors, in order: RTO_E_INVALID (n < 0, or
 * n > 0 with a NULL pointer; 8- and 4-byte alignment), RTO_E_NO_OCTREE, RTO_E_UNSUPPORTED (no resident grid).  n == 0 is RTO_OK. */
int  rto_query_dual_vertices_device(rto_context* ctx, const int64_t* d_voxels, int64_t n, rto_dual_vertex* d_out);
int  rto_query_dual_vertices_host(rto_context* ctx, const int64_t* voxels, int64_t n, rto_dual_vertex* out);

/* ---- instrumentation ------------------------------------------------------*/
/* Renders the frame once with counting enabled (synchronous). */
int  rto_frame_stats(rto_context* ctx, const rto_frame* frame, rto_stats* out);
/* Per-pixel traversalSteps: +steps for a hit, -steps for a miss (width*height int32, host). */
int  rto_render_steps_host(rto_context* ctx, const rto_frame* frame, int32_t* host_steps);
/* Developer aid: per-wave timeline of one frame of the packed kernel.  8 int32 per 8x8 tile (row-major
 * tiles): start lo/hi, end lo/hi (100 MHz wall clock), loop iterations, HW_ID, XCC_ID, lanes that entered
 * the tree | launch slot << 8; all zero for tiles outside the root rectangle's tile box, which get no wave (their pixels are written
 * by the waves of the box as wide stores).  host_records may be NULL to query *num_tiles. */
int  rto_debug_timeline(rto_context* ctx, const rto_frame* frame, int32_t* host_records, int64_t capacity_tiles,
                        int64_t* num_tiles);
/* Developer aids for the launch-order study: per-tile trip counts of the last frame, and a caller-supplied
 * slot -> tile table (NULL restores the automatic one). */
int  rto_debug_tile_cost(rto_context* ctx, int32_t* host_cost, int64_t capacity, int64_t* count);
int  rto_debug_set_tile_order(rto_context* ctx, const int32_t* host_order, int64_t n);
/* The occupancy mask: the first few workgroups of every colour / shade frame of the default kernels
 * project the octree's coarse cells (its internal nodes at one depth + the solid leaves above it) onto the screen and stamp
 * the 8x8 tiles they can touch; once the mask is complete, waves of unstamped tiles write black without setting up a single
 * ray (about two thirds of the rays inside the geometry's screen rectangle miss everything).  Nobody waits for the mask: the
 * previous frame's costliest tiles never look, later waves look only if it is complete -- tiles without work sort to the end
 * of the launch order, where it always is.  A scheduling device like the launch order: pixels never depend on it.
 * rto_debug_set_tile_mask: 0 = off, 1 = on (default), 2 = on and built by a launch of its own in front of the frame, every
 * wave consulting it (tests: the mask decides for every tile).  _info: the depth the cells are taken from and their number
 * (0: no mask for this octree). */
int  rto_debug_set_tile_mask(rto_context* ctx, int enabled);
int  rto_debug_tile_mask_info(const rto_context* ctx, int* level, int* num_cells);
/* Test hook: from now on the k-th (1-based) allocation of the frustum-update / rto_comm buffers of this PROCESS fails (k <= 0: never).
 * An explicit call -- the library reads no environment variable (A/B knobs exist only in -DRTO_DEV_KNOBS builds). */
int  rto_debug_fault_alloc(long k);
/* Writes the launch-order sort refused because they fell outside the table (must be 0; synchronises). */
int  rto_debug_sort_violations(rto_context* ctx, int* count);
/* Device time in ms of the most recent traversal kernel launched by this context
 * (hipEvent pair on the launch stream; synchronises on that event). */
int  rto_last_kernel_ms(rto_context* ctx, float* ms);
/* Per-launch timing without synchronising inside a timed loop: after rto_timing_begin(ctx, n) the next n
 * traversal-kernel launches are bracketed by their own hipEvent pair on the launch stream (just that kernel: the
 * launch-order kernel that may follow is outside the pair); rto_timing_read synchronises the device and returns the
 * durations in ms.  rto_timing_begin(ctx, 0) switches it off (rto_last_kernel_ms keeps working: one event pair per launch).
 * rto_timing_begin(ctx, -1) records no events at all until the next rto_timing_begin(ctx, >= 0): an event costs ~2 us
 * between two dependent launches, which matters when frames of ~50 us are issued back to back without a HIP graph. */
int  rto_timing_begin(rto_context* ctx, int capacity);
int  rto_timing_read(rto_context* ctx, float* ms, int capacity, int* count);   /* ms may be NULL to query count */
/* The context's own hipStream_t (used by the synchronous entry points). */
void* rto_stream(rto_context* ctx);
/* Waits for all work on the context's device (hipDeviceSynchronize). */
int  rto_synchronize(rto_context* ctx);

#ifdef __cplusplus
}
#endif
#endif
