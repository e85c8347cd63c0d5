// laserMapping on gfx950 — host-visible interface of the map_*.hip files (the prototypes at the end are grouped by implementing file).
//
// The reference keeps 21x21x11 cubes of pcl clouds, gathers the 5x5x3 block around the sensor, builds
// two kd-trees per sweep and re-voxelises every valid cube (laser_mapping.cpp:198-708).  Here the map
// is a PERSISTENT voxel hash in HBM keyed by (absolute cube, voxel inside the cube), one slot per
// per-cube VoxelGrid cell, holding the cell's f32 running sum + count — which reproduces the
// reference's "centroid of (old centroid, new points...)" update exactly (SURVEY.md §8a map notes)
// with no per-sweep gather / tree build / re-sort.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/vloam_hip/c_api.h"
#include "sr_kernels.h"
#include "vloam_device.h"

namespace vloam {

constexpr int kCubeW = 21, kCubeH = 21, kCubeD = 11, kCubeNum = kCubeW * kCubeH * kCubeD;  // laser_mapping.h:110-117
constexpr int kStackCapCorner = 8192;   // >= kMaxLessSharp
constexpr int kStackCapSurf = 24576;    // voxels of one sweep's lessFlat cloud at the plane resolution (with the corner stack: 32 768 slots = the 512 mask rows of a solve)
constexpr int kMapFactorCap = kStackCapCorner + kStackCapSurf;
// Large stack tier (vloam_limits::max_surf_stack_points): a handle may size its surf stack — and everything indexed by a stack slot — up to
// kStackCapSurfMax in steps of kStackCapSurfStep.  Corner slots stay [0, kStackCapCorner), surf slots behind them.  Such a handle launches the
// *_tier forms of the kernels that bake the constants above in (map_kernels.hip, map_prepare_fit.inc.h) and solves in the packed form (more than 512 mask rows).
constexpr int kStackCapSurfStep = 8192, kStackCapSurfMax = 131072;
static_assert(kStackCapSurfMax <= (1 << 17), "the tier's raw-point arrival stamp keeps 17 bits of stack index (k_map_finalize_tier)");
constexpr int kPendCap = 16;            // stack points that may land in one map voxel in one sweep
// Voxel indices one axis of a 50 m cube can take at a leaf of 1 / inv (+ slack: the first index of a cube is taken one cell early, and the
// cube test runs in f64 on the point while the voxel index is an f32 product): the radix of k_map_assoc's 32-bit tie rank — the position of
// a voxel in the reference's gathered map cloud, 75 cubes x radix^3.  vloam_create keeps 75 radix^3 below 2^32 (leaf >= 0.132 m); the
// voxel key itself has 9 bits per axis (map_table.h).
__host__ __device__ inline int vox_radix(float inv) { return (int)(50.0f * inv) + 4; }

// One map voxel == one 32-byte record, so that a candidate of the 5-NN search, an insert and a finalize each touch ONE cache line
// (round 1 kept keys / sums / counts in three arrays: three scattered lines per candidate, 27x the algorithmic traffic).
struct __attribute__((aligned(32))) VoxelRec {
  unsigned long long key;    // 0 = empty
  float sx, sy, sz, si;      // f32 running sum (x, y, z, intensity) in arrival order
  int count;                 // points in the sum (1 after a valid-cube finalize; 0 = purged, or created this sweep and not finalized yet)
  int pend_cnt;              // stack points queued this sweep
};
static_assert(sizeof(VoxelRec) == 32, "one voxel, one half cache line");

struct VoxelTable {       // open addressing, linear probing, probe chains bounded by kMaxProbe
  VoxelRec* rec;
  int* pend;                 // [slots][kPendCap] stack indices
  unsigned mask;             // slots - 1
  // occupancy index: one entry per 4 x 4 x 4 block of voxels of a cube -> 64-bit mask of the voxels that exist.
  // The 5-NN search probes ~27 blocks instead of ~343 mostly empty voxels.
  ulonglong2* blk;           // {key (0 = empty), mask}: one 16-byte load per probe
  unsigned bslots_mask;      // block slots - 1
  int* stats;                // [4] keys in the table (live + purged) | entries purged since the last rebuild | block keys | spare
  __host__ __device__ void rebase(size_t off) { rbp(rec, off); rbp(pend, off); rbp(blk, off); rbp(stats, off); }
};
constexpr int kMaxProbe = 128;  // a longer chain means the table is overloaded: the lookup reports kErrMapFull instead of spinning
constexpr int kCandChunk = 256; // candidate lists longer than this are reported in MapFrame::max_candidates (the 5-NN search takes them in several passes, exactly)
constexpr int kCandCache = 128; // entries per stack point in the second outer round's candidate cache (>= the pass size of every lane count of k_map_assoc)

// scan-feature VoxelGrid (k_map_ds_bin / k_map_ds_reduce): the cell-index space of a sweep's cloud is cut into bins of ~kDsBinTarget points
constexpr int kDsMaxBins = 256;      // bins per cloud (a cloud of more than 256 x 512 points gets fuller bins)
constexpr int kDsBinTarget = 512;    // points per bin aimed at
constexpr int kDsBinCap = 4096;      // keys a bin's region holds == keys the reduce pass sorts in LDS; a fuller bin spills into the overflow list
constexpr int kDsBigCell = 32;       // cells with more points than this are folded by a whole wavefront
constexpr int kDsBigCap = 128;       // such cells per bin (4 096 / 33)

struct DsScratch {        // per-sweep VoxelGrid of the scan features (laser_mapping.cpp:432-440)
  unsigned long long* region;     // [kDsMaxBins][kDsBinCap] sort keys (cell index << 24 | point index) by bin, arrival order inside a bin
  unsigned long long* over;       // [max_points] keys that found their bin's region full
  unsigned long long* tmp;        // [max_points] slow path: an over-full bin gathered from its region + the overflow list ...
  unsigned long long* sorted;     // [max_points] ... and ranked
  unsigned long long* splitters;  // [kDsMaxBins] this sweep's bin boundaries (cell indices)
  int* cursor;                    // [kDsMaxBins] keys per bin | [kDsMaxBins] overflow entries | [+1] ticket of the reduce pass | [+2] slow-path scratch in use
  unsigned long long* done;       // [kDsMaxBins] look-back words: sweep generation << 32 | cells of the bin
  int stack_cap;
  __host__ __device__ void rebase(size_t off) {
    rbp(region, off); rbp(over, off); rbp(tmp, off); rbp(sorted, off); rbp(splitters, off); rbp(cursor, off); rbp(done, off);
  }
};

struct StackInfo {        // per stack set: counters of the scan-feature VoxelGrid (written on its own stream)
  int n_stack[2];         // laserCloudCornerStackNum / laserCloudSurfStackNum
  int error;
};

struct MapFrame {         // per-sweep device counters
  int n_uniq[2];
  int n_stack[2];
  int n_touched[2];
  int n_deferred[2];
  int n_newraw[2];        // voxels that turned raw this sweep (merged into the deferred list by the next k_map_prepare)
  int rolled;
  int error;
  int n_factors[2][2];    // [outer][corner, surf] accepted factors
  int max_candidates;     // largest 5-NN candidate list seen (diagnostic; lists beyond kCandChunk take extra passes)
  int fallback_solves;    // cooperative Levenberg-Marquardt solves of this session that degraded to one workgroup (lm_solve.hip)
};

// The clouds of LaserMapping::publish as products of the mapping stream (vloam_limits::map_pub_number / publish_registered_cloud; LM:778-805).
// Everything here lives in the session arena and only on a handle that asked for it.  /laser_cloud_map is ordered on the device: the live
// records are counted per (cube, kind) bucket, an exclusive scan turns the counts into segment offsets, the records are scattered into their
// segments, and every segment is ordered by its key — in LDS when it fits (kPubLdsKeys), by counting smaller keys otherwise.  A point's
// place is a function of the keys alone.
constexpr int kPubBuckets = 2 * kCubeNum;   // (cube, kind): the leading bits of the order key
constexpr int kPubLdsKeys = 4096;           // segments of up to this many records are sorted in LDS by one workgroup (k_map_pub_sort)
constexpr long long kPubMapCapDefault = 2097152, kPubMapCapMin = 256, kPubMapCapMax = 16777216;
struct PubHeader { long long n; int overflow; int pad; };   // next to each publication buffer: true count | 1 = more than the capacity, nothing written
struct MapPub {
  int pub_number = 0;          // vloam_limits::map_pub_number
  int skip_n = 1;              // vloam_config::mapping_skip_frame
  bool due(int frame_count) const { return ((long long)frame_count * skip_n) % pub_number == 0; }   // LM:778, frameCount = mapped sweeps so far
  long long cap = 0;           // vloam_limits::max_published_map_points
  int cloud_on = 0;            // vloam_limits::publish_registered_cloud
  int* cnt = nullptr;          // [kPubBuckets] records per bucket (zero between publications: k_map_pub_sort clears what it has read)
  int* off = nullptr;          // [kPubBuckets + 1] exclusive scan of cnt
  int* cur = nullptr;          // [kPubBuckets] scatter cursors
  unsigned long long* keys = nullptr;   // [cap] order keys by segment, arrival order inside a segment
  float4* vals = nullptr;      // [cap] their points
  float4* out[2] = {nullptr, nullptr};       // [cap] the ordered cloud, two publications
  PubHeader* hdr[2] = {nullptr, nullptr};
  float4* cloud[2] = {nullptr, nullptr};     // [max_points] registered full-resolution cloud, two publications
  int* cloud_n[2] = {nullptr, nullptr};      // its count (the sweep's FrameScalars::N2)
  // host side
  hipEvent_t ev_map[2] = {nullptr, nullptr}, ev_cloud[2] = {nullptr, nullptr};   // recorded behind each publication
  int map_seq = 0, cloud_seq = 0;            // publications enqueued so far (the latest sits in buffer (seq - 1) & 1)
  int map_frame[2] = {-1, -1}, cloud_frame[2] = {-1, -1};
  int mapped = 0;              // mapped sweeps enqueued (map_enqueue counts them) == MapState::sweep_no once they have run
  void rebase(size_t o) {
    rbp(cnt, o); rbp(off, o); rbp(cur, o); rbp(keys, o); rbp(vals, o);
    for (int k = 0; k < 2; k++) { rbp(out[k], o); rbp(hdr[k], o); rbp(cloud[k], o); rbp(cloud_n[k], o); }
  }
};

// Growable map (vloam_map_options::grow, single-sequence handles): the two tables' rec / pend / blk live in allocations of their own and are
// rehashed into larger ones between two sweeps (k_map_grow); a handle without the option has no MapGrow at all.  The host decides on a BOUND,
// not on a count (map_enqueue): last reported keys + (mapped sweeps enqueued since that report) x (what one sweep can add).
struct MapGrow {
  int max_log2 = 28;              // ceiling per table: there k_map_finalize's kErrMapFull returns
  int lg[2] = {0, 0};             // current log2 of the corner / surf table
  long long steps = 0;            // growth steps enqueued so far, both tables
  long long inc_rec[2] = {0, 0};  // records / block keys one mapped sweep can add to a table at most (set at creation, c_api.cpp)
  long long inc_blk[2] = {0, 0};
  unsigned long long* progress = nullptr;   // host-mapped [2 kinds][3]: sweep << 32 | live keys, | block keys, | keys incl. tombstones (k_map_progress)
  long long step_at[2] = {-1, -1};  // mapped sweeps enqueued when the table was last rehashed: reports up to that sweep still count its tombstones
  static constexpr int kEvRing = 4;
  hipEvent_t ev_prog[kEvRing] = {};   // behind k_map_progress of mapped sweep n (slot n % kEvRing): the only thing the growth decision may wait for
  int failed_log2 = 0;            // > 0: the last step could not allocate a table of that size (the caller words the error and clears it)
  struct Retired { void* p[3]; hipEvent_t ev; };
  std::vector<Retired> retired;   // buffers a grow chain still reads: released once their event has fired (map_grow_release)
  std::vector<void*> leftover;    // what a failed allocation had got already: freed by map_grow_release (hipFree synchronises the device)
};

// Scratch of a localisation (vloam_map_localize; map_localize.hip): a dry run of the mapping chain works on its own MapState / MapFrame, stacks,
// factor tables and candidate cache.  One allocation of its own, made by the first call, outside the session arena; null on a handle that never localises.
struct LocAux { int shift[3]; int si_error; double guess[7]; };   // k_map_loc_prepare -> k_map_loc_finish
struct MapLocalize {
  char* base = nullptr;            // the allocation
  MapState* state = nullptr;
  MapFrame* frame = nullptr;
  LocAux* aux = nullptr;
  StackInfo* si = nullptr;         // foreign clouds: counters of their VoxelGrid
  FrameScalars* S = nullptr;       // ... and its counts / bounding boxes (k_sr_adopt)
  float4* in[2] = {nullptr, nullptr};      // the host form's uploaded clouds
  float4* stack[2] = {nullptr, nullptr};
  DsScratch ds[2];
  unsigned ds_gen = 0;
  FactorTable F[2];
  LMRecord* rec = nullptr;         // [2]
  float4* nbr = nullptr;
  int4* cbox = nullptr;
  float4* ccand = nullptr;
  vloam_localize_result* result = nullptr;   // the host form's record
};

// Map clean-up (vloam_map_carve; map_carve.hip): what one call's kernels share.  The scratch — poses, counters, range images, uploaded sweeps and
// the removed list — is one allocation of its own made by the first call and regrown when a call needs more; null on a handle that never carves.
struct CarveGeom {        // the projection into the range image, f32 as c_api.h states it (set on the host: carve_geom)
  int rows, cols, n_sweeps, min_votes;
  float min_range, max_range, range_res;
  float elev_min, row_scale, col_scale;
  unsigned margin_q;
};
struct CarvePose { double R[9], t[3]; };   // map <- sensor: p_map = R p_s + t (row-major R, from the normalised quaternion)
constexpr int kCarveMaxSweeps = 16, kCarveMaxPoints = 262144, kCarveMaxPixels = 1 << 20;
constexpr int kCarveCounters = 6;          // examined, in_view, seen_through, confirmed, removed, skipped_raw
struct CarveCounters { unsigned long long cnt[2][kCarveCounters]; unsigned long long n_removed; };
struct MapCarve { char* base = nullptr; size_t bytes = 0; };
// Map merge (vloam_map_merge; map_merge.hip): this map <- the clouds' frame, p' = R p + t (row-major R from the normalised quaternion, set on
// the host as CarvePose's).  identity: q = (0, 0, 0, 1) and t = 0, the points are taken as they are
struct MergeXf { double R[9], t[3]; int identity; };

// Map archive (vloam_map_archive_enable; map_archive.hip): the rows of evicted points and their counters, one allocation of its own; null on a
// handle that never enabled it.  frame: the sweep map_enqueue is about to be called for (set by its caller; the rows carry it)
struct MapArchive {
  char* base = nullptr;
  int* cnt = nullptr;                      // [4] rows held | rows dropped since the last clear | rolls seen | -
  vloam_map_archive_row* rows = nullptr;   // [cap]
  long long cap = 0;
  int frame = 0;
};

struct MapContext {
  MapState* state = nullptr;
  MapFrame* frame = nullptr;
  VoxelTable tab[2];       // 0 corner, 1 surf
  int* cube_cnt = nullptr; // [2][kCubeNum] points per cube, window-relative index (== the reference's array index)
  DsScratch ds[2];
  unsigned ds_gen = 0;      // scan-feature VoxelGrids enqueued so far (tags the look-back words of k_map_ds_reduce)
  static constexpr int kSets = kBufferSets;   // == the SR buffer sets of the handle (same rotation)
  float4* stack_sets[kSets][2] = {};          // laserCloudCornerStack / laserCloudSurfStack (sensor frame), one pair per set
  StackInfo* stack_info[kSets] = {};
  float4* stack[2] = {nullptr, nullptr};      // the pair of the sweep mapping is working on (host-side alias)
  float4* stack_map[2] = {nullptr, nullptr};  // the same points in the map frame (at insert time)
  int* touched[2] = {nullptr, nullptr};       // table slots that received points this sweep
  int* deferred[2] = {nullptr, nullptr};      // slots of the raw voxels (points that arrived while their cube was outside the valid block)
  int* newraw[2] = {nullptr, nullptr};        // ... the ones that turned raw in the sweep being finalized
  FactorTable F[2];        // one per outer round (kept for the parity hooks)
  LMRecord* rec = nullptr; // [2]
  int surf_cap = kStackCapSurf;   // capacity of laserCloudSurfStack of this handle (set before map_layout); > kStackCapSurf: the large stack tier
  int factor_cap() const { return kStackCapCorner + surf_cap; }   // slots of everything below that is indexed by a stack slot
  bool tier() const { return surf_cap > kStackCapSurf; }
  float4* nbr = nullptr;   // [factor_cap()][5] the 5 nearest map points of every stack point (.w of the first: 1 = accepted, LM:479 / LM:547)
  int4* cbox = nullptr;    // [factor_cap()][2] voxel-index search box + candidate count of the first outer round's 5-NN search
  float4* ccand = nullptr; // [factor_cap()][pass size <= kCandCache] its candidates (centroid, tie rank): the second round re-ranks them without a hash probe
  VoxelRec* rebuild_tmp = nullptr;  // live records while a table is being rebuilt (tombstone reclamation after grid rolls)
  int rebuild_cap = 0;
  int* rebuild_n = nullptr;
  int* host_flags = nullptr;        // host-mapped: [kind] 1 = the table of that kind wants a rebuild (written by k_map_finalize)
  int rebuild_cooldown[kMaxBatch][2] = {};
  long long rebuilds = 0;
  MapGrow* grow = nullptr; // growable map: null on every handle that did not ask for it.  Such a handle has ONE session, so for_session's
                           // rebase of tab[] is by zero and tab[] always names the current buffers for every reader
  Sess se;                 // sessions of the handle (launch geometry .z and arena stride)
  int sel = 0;             // session the host-side getters read (vloam_select_session)
  // a copy whose device pointers address session b (host-side getters, per-session rebuilds)
  MapContext for_session(int b) const {
    MapContext m = *this;
    const size_t off = (size_t)b * se.ss;
    rbp(m.state, off); rbp(m.frame, off); m.tab[0].rebase(off); m.tab[1].rebase(off); rbp(m.cube_cnt, off); m.ds[0].rebase(off); m.ds[1].rebase(off);
    for (int c = 0; c < kSets; c++) { rbp(m.stack_sets[c][0], off); rbp(m.stack_sets[c][1], off); rbp(m.stack_info[c], off); }
    for (int k = 0; k < 2; k++) { rbp(m.stack[k], off); rbp(m.stack_map[k], off); rbp(m.touched[k], off); rbp(m.deferred[k], off); rbp(m.newraw[k], off); m.F[k].rebase(off); }
    rbp(m.rec, off); rbp(m.nbr, off); rbp(m.cbox, off); rbp(m.ccand, off); rbp(m.registered, off); rbp(m.assoc_cyc, off); rbp(m.ts_log, off); rbp(m.rebuild_tmp, off); rbp(m.rebuild_n, off);
    if (m.host_flags) m.host_flags += 2 * b;
    m.pub.rebase(off);
    m.se.B = 1; m.sel = 0;
    return m;
  }
  MapLocalize* loc = nullptr;   // localisation scratch: null until the first vloam_map_localize* call (host-side; not rebased: single-sequence handles only)
  MapCarve* carve = nullptr;    // map clean-up scratch: null until the first vloam_map_carve* call (host-side, like loc)
  MapArchive* archive = nullptr;   // map archive: null until vloam_map_archive_enable (host-side, like loc)
  MapPub pub;              // published clouds (off on a default handle)
  float4* registered = nullptr;  // full-resolution cloud in the map frame, on request
  long long* assoc_cyc = nullptr;  // [2][8] debug: phase cycle sums of k_map_assoc per outer round
  long long* ts_log = nullptr;     // [1024][2] VLOAM_TS_LOG=1: constant-rate (100 MHz) clock at the start of k_map_prepare / end of k_map_finalize of sweep k % 1024
  int max_points = 0;
  float inv_leaf[2] = {0, 0};
};

// ---- map_kernels.hip: the mapping chain and its state
// layout: carve the session arena (called twice: dry to measure, then for real); init: the initial device state of session 0
vloam_status map_layout(MapContext* m, const vloam_config& cfg, Arena& A);
vloam_status map_init(MapContext* m, hipStream_t st);
vloam_status map_enqueue(MapContext* m, const vloam_config& cfg, hipStream_t st, const SRBuffers& cur, LOState* lo, double* traj_row14,
                         bool skip_frame, int set, ProfHook* ph, hipEvent_t done = nullptr);
vloam_status map_force_rebuild(MapContext* m, hipStream_t st);  // every session
vloam_status map_reclaim_enqueue(MapContext* m, hipStream_t st, int kind);   // one table of a single-sequence handle: rebuild (fixed) or same-size rehash (growable)
void map_destroy(MapContext* m);
// ---- map_stack.hip: the scan-feature VoxelGrid, enqueued on the scan-registration stream
vloam_status map_stack_enqueue(MapContext* m, hipStream_t st, const SRBuffers& cur, int set, ProfHook* ph, hipEvent_t done = nullptr);
// ---- map_output.hip: what a caller reads of the map and of a sweep's clouds
vloam_status map_get_cloud(MapContext* m, hipStream_t st, int which, const SRBuffers& cur, float* xyzi4, int cap, int* n);
// == /laser_cloud_map (laser_mapping.cpp:778-793): every cube's corner cloud then surf cloud, cube index ascending
vloam_status map_export(MapContext* m, hipStream_t st, float* xyzi4, long long cap, long long* n);
// the corner (0) or surf (1) half of it, same order within the half
vloam_status map_export_kind(MapContext* m, hipStream_t st, int kind, float* xyzi4, long long cap, long long* n);
// Publications of sweep `frame`, enqueued on the mapping stream behind map_enqueue of that sweep: the registered cloud first, then `done`
// (non-null on a handle with the registered cloud, whose map_enqueue was given done == nullptr: k_map_register still reads the sweep's buffer
// set), then the map, which reads the voxel tables only.  cloud / S: the sweep's laserCloudFullRes and its scalars, session 0's addresses.
// No allocation, host copy or synchronisation.
bool map_publishes(const MapContext* m, bool skip_frame);   // asked BEFORE map_enqueue of the sweep: will it publish anything?
vloam_status map_publish_enqueue(MapContext* m, hipStream_t st, const float4* cloud, const FrameScalars* S, int frame, bool skip_frame, ProfHook* ph,
                                 hipEvent_t done);
// which: 0 map, 1 registered cloud; the latest publication of the selected session.  Waits for that publication's event only.
// d_ptr (may be NULL): its device address.  xyzi4 (may be NULL): host buffer of cap points.  VLOAM_ERR_CAPACITY: the map overflowed (*n = true count).
vloam_status map_published_get(MapContext* m, int which, float* xyzi4, long long cap, long long* n, int* frame, void** d_ptr);
// ---- map_inspect.hip: host inspection (sticky error words, parity hooks, counts)
vloam_status map_error(MapContext* m, int* err_bits, int clear_mask = 0, long long* fallback_solves = nullptr);
vloam_status map_debug_get(MapContext* m, int item, void* buf, long long cap, long long* n);
vloam_status map_counts(MapContext* m, long long c[16]);
// ---- map_query.hip (a code object of its own): the k <= 8 nearest map points within `radius` of n query points (device addresses, map frame) of the
// selected session, kind 0 corner map / 1 surf map / 2 both.  Enqueue only, no allocation: d_xyzi4 [n][k] float4, d_d2 [n][k], d_count [n].
vloam_status map_query_enqueue(MapContext* m, hipStream_t st, int kind, int k, float radius, const void* d_xyz_pad4, int n, void* d_xyzi4, void* d_d2,
                               void* d_count);
// ---- map_score.hip (a code object of its own): hits and quantised nearest-neighbour distances of n_corner / n_surf sensor-frame points (device
// addresses, every stride[kind]-th point) under M poses (device address, [M][7] f64: q xyzw, t) against the corner / surf map of a single-sequence
// handle.  Enqueue only, no allocation: d_out [M] vloam_pose_score, zeroed and filled on st.
vloam_status map_score_enqueue(MapContext* m, hipStream_t st, const void* d_corner, int n_corner, const void* d_surf, int n_surf, const int stride[2],
                               const float radius[2], const double* d_q4t3, int M, void* d_out);
// ---- map_localize.hip (a code object of its own) + map_localize_enqueue in map_kernels.hip, beside map_enqueue: a dry run of the mapping chain
// on scratch state (vloam_map_localize).  Single-sequence handles of the default stack tier.  corner / surf: device clouds (sensor frame), or both
// null: stack set `set` as map_stack_enqueue left it, read-only.  row7: device address of an odometry pose (q xyzw, t), or null: pose7 (host
// values, passed by value).  pose_frame 1: the pose is the guess itself.  d_result: device address the record is packed into.
vloam_status map_localize_alloc(MapContext* m, hipStream_t st);   // first call: the scratch, zeroed on st; VLOAM_ERR_HIP when the allocation fails
void map_localize_free(MapContext* m);
vloam_status map_localize_enqueue(MapContext* m, hipStream_t st, const float4* corner, int n_corner, const float4* surf, int n_surf, int set,
                                  const double* row7, const double pose7[7], int pose_frame, vloam_localize_result* d_result);
// the two kernels of map_localize.hip, launched by map_localize_enqueue
void map_loc_prepare_launch(hipStream_t st, const MapContext* m, const StackInfo* si, const double* row7, const double pose7[7], int pose_frame);
void map_loc_finish_launch(hipStream_t st, const MapContext* m, vloam_localize_result* d_result);
// map_stack.hip: the scan-feature VoxelGrid of foreign clouds into the localisation scratch (the kernels and grids of map_stack_enqueue)
void map_stack_enqueue_loc(MapContext* m, hipStream_t st, const float4* corner, const float4* surf);
// ---- map_import.hip (a code object of its own): vloam_map_import.  On the empty tables of a fresh single-sequence handle, nothing in flight: the window
// is placed for pose7 (q xyzw, t: the map<-odometry transform), cloud[kind] (n[kind] packed float4 in the map frame; host memory with host_clouds,
// else device memory) is keyed, merged per voxel in input order and inserted.  Temporary allocations only; synchronises st and frees them.
// h_result: host memory.  The sticky map-full error is the caller's to read (MapFrame::error).
vloam_status map_import_run(MapContext* m, hipStream_t st, const double pose7[7], const void* const cloud[2], const int n[2], bool host_clouds,
                            vloam_map_import_result* h_result);
// ---- map_merge.hip (a code object of its own): vloam_map_merge.  On the tables of a single-sequence handle, live or fresh, nothing in flight: cloud[kind]
// (n[kind] packed float4 in the other map's frame; host memory with host_clouds, else device memory) goes through X into this map's frame, is keyed
// against the current window and folded per voxel in input order onto what the voxel holds (apply), or only looked up (dry run).  Temporary
// allocations only; synchronises st and frees them.  place_start: the window was never placed (map_window_never_placed) — an applied call then
// starts the handle at the identity as an import would.  h_result: host memory.  The sticky map-full error is the caller's to read (MapFrame::error).
vloam_status map_merge_run(MapContext* m, hipStream_t st, const MergeXf& X, const void* const cloud[2], const int n[2], bool host_clouds, bool apply,
                           bool place_start, vloam_map_merge_result* h_result);
// no sweep mapped, nothing imported or restored: the centre cube was never set (a placed one lies in [3, kCube - 3) on every axis)
inline bool map_window_never_placed(const MapState& s) { return s.sweep_no == 0 && s.centerCube[0] == 0 && s.centerCube[1] == 0 && s.centerCube[2] == 0; }
// ---- map_carve.hip (a code object of its own): vloam_map_carve.  With nothing of the handle in flight, on st: range images of the sweeps
// (clouds[s]: n[s] packed float4, host memory with host_io, else device addresses), the vote over the records of the kinds in kind_mask of session
// `session`, the removed points into `removed` (cap points; host memory with host_io) and, with apply (single-sequence handles), the removal and the
// tables' reclamation.  Waits for st.  h_out: the counters; n_removed > cap: nothing was applied.
vloam_status map_carve_run(MapContext* m, int session, hipStream_t st, const CarveGeom& G, int kind_mask, const void* const* clouds, const int* n,
                           const CarvePose* poses, bool host_io, void* removed, long long cap, bool apply, CarveCounters* h_out);
void map_carve_free(MapContext* m);
// ---- map_archive.hip (a code object of its own): vloam_map_archive_*.  alloc: rows + counters, zeroed on st and waited for.  enqueue: k_map_archive
// on st, for map_enqueue — between k_map_prepare and k_map_finalize of a mapped sweep of a single-sequence handle with m->archive set.
vloam_status map_archive_alloc(MapContext* m, hipStream_t st, long long capacity_rows);
void map_archive_free(MapContext* m);
void map_archive_enqueue(const MapContext* m, hipStream_t st);
// ---- map_grow.hip: growable handles (m->grow != null).  map_force_grow: test hook, one doubling of both tables now (between two sweeps, on the mapping stream).
// map_grow_release: frees retired buffers whose grow chain has finished (hipEventQuery); call with nothing of the handle in flight — hipFree
// synchronises the device.
vloam_status map_force_grow(MapContext* m, hipStream_t st);
void map_grow_release(MapContext* m);
// the rest of map_grow.hip's interface, for map_kernels.hip (map_layout / map_init / map_destroy / map_enqueue): the tables' first allocation / everything the option owns; a rehash of table
// `kind` at its size (tombstone reclamation); the growth decision in front of a mapped sweep; k_map_progress behind its k_map_finalize
vloam_status map_grow_init(MapContext* m, hipStream_t st);
void map_grow_destroy(MapContext* m);
vloam_status map_grow_rehash(MapContext* m, hipStream_t st, int kind);
vloam_status map_grow_before_sweep(MapContext* m, hipStream_t st);
void map_grow_progress_enqueue(MapContext* m, hipStream_t st);
// ---- map_ckpt.hip, map_grow.hip: checkpoint of a sequence (vloam_checkpoint_save / _load; single-session handles, nothing in flight).  map_ckpt.hip: the live records of both
// tables counted (n_rec) and, with d_out, packed into a device buffer the caller frees — corner records, then surf records; the reverse into the
// empty tables of a fresh handle from host memory.  ms (may be null): kernel times, {count + scan, pack} / unpack.  map_grow.hip: what a
// growable handle does first (the table size its growth bound asks for; the step to it and the report words).
vloam_status map_ckpt_pack(MapContext* m, hipStream_t st, long long n_rec[2], VoxelRec** d_out, float ms[2]);
vloam_status map_ckpt_unpack(MapContext* m, hipStream_t st, const void* recs, const long long n_rec[2], float* ms);
int map_grow_restore_log2(const MapContext* m, int kind, long long live, long long blk);
vloam_status map_grow_restore(MapContext* m, hipStream_t st, const int lg[2], const long long live[2], const long long blk[2], long long mapped);

}  // namespace vloam
