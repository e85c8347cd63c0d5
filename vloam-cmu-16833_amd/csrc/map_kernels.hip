// laserMapping on gfx950: scan-to-map ICP against a persistent voxel hash — the mapping chain, which sets the sweep period, and what owns its state.
// Restates LaserMapping::input / solveMapping, the reference's src/lidar_odometry_mapping/src/laser_mapping.cpp:167-708
// ("LM:<line>").  One sweep = 11 launches incl. 2 Levenberg–Marquardt solves (which compact on their own), no host synchronisation; the two
// k_map_ds_* launches (map_stack.hip) only need the sweep's feature clouds and run on a stream of their own.  Every kernel carries the session
// index of a batched handle in blockIdx.z and rebases its pointer arguments by blockIdx.z * ss (vloam_device.h).
//   k_map_prepare   1 WG      initial guess (LM:193-194), centre cube + grid roll (LM:207-402), gate (LM:448); stops taking sweeps
//                             when the voxel table is full
//   k_map_assoc     1 wave/pt pointAssociateToMap, exact 5-NN through the block-occupancy index of the voxel hash (one 32-byte
//                             record per candidate); the second outer round re-ranks the first round's candidates             x2
//   k_map_fit       1 thread/pt 3x3 eigen / 5x3 least squares, emission of LidarEdgeFactor / LidarPlaneNormFactor (LM:472-581) x2
//   (k_lm_solve)                                                                                                x2
//   k_map_insert    grid      transformUpdate (LM:140-144,636) + trajectory row; scan voxels -> map frame -> cube -> hash
//                             find-or-insert, queue on the voxel (LM:639-683)
//   k_map_finalize  grid      per touched voxel: stack-ordered f32 accumulation == per-cube VoxelGrid re-filter (LM:689-702);
//                             raw voxels of cubes that became valid; after a grid roll drops the voxels whose cube left the
//                             21x21x11 window (tombstones); table health -> host-mapped rebuild flag
//   k_map_rebuild_* grid      (rare, between sweeps) gather live records, clear, reinsert: tombstone reclamation
//   (map_stack.hip)           k_map_ds_bin / k_map_ds_reduce: pcl::VoxelGrid of the scan features (LM:432-440), on the scan-registration stream
//   (map_grow.hip)            growable handles: k_map_grow rehashes a table into a fresh one between sweeps, k_map_progress reports its keys
//   (map_output.hip)          k_map_register, k_map_export, k_map_pub_*: vloam_get_map, vloam_get_features(h, 11), the published clouds
//   (map_query.hip)           k_map_query: the k nearest map points of caller-supplied points, on request (vloam_map_query)
//   (map_inspect.hip)         host inspection: sticky error words, parity hooks (map_debug_get), counts
//   (map_device.h)            the device helpers these files share
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <type_traits>
#include "lm_solve.h"
#include "map_kernels.h"
#include "map_device.h"
#include "map_table.h"
#include "map_move_dev.h"
#include "subwave.h"

namespace vloam {

// ---------------------------------------------------------------------------------------------- prepare
// k_map_prepare (and, below, k_map_fit): map_prepare_fit.inc.h, included once per form further down
// Drop voxels whose cube left the window (the reference clears the slab that wraps, LM:240-241 etc.).  Only after a roll.
// The window is +-500 m around the sensor while queries and inserts stay within the +-125 m valid block, so nothing of the
// sweep that rolled can touch such a voxel: the sweep's last launch (k_map_finalize) does the purge on its way out, instead
// of a launch of its own in front of the association.
__device__ void map_purge(const VoxelTable& T, const MapState* ms, int first, int stride) {
  const int cW = ms->cenW, cH = ms->cenH, cD = ms->cenD;
  int dead = 0;
  for (unsigned s = (unsigned)first; s <= T.mask; s += (unsigned)stride) {
    const RecVal v = rec_load(&T.rec[s]);
    if (v.key == 0 || v.count == 0) continue;
    int Ai, Aj, Ak;
    unpack_cube(v.key, &Ai, &Aj, &Ak);
    const int i = Ai + cW, j = Aj + cH, kk = Ak + cD;
    if (i < 0 || i >= kCubeW || j < 0 || j >= kCubeH || kk < 0 || kk >= kCubeD) { rec_store_value(&T.rec[s], make_float4(0.f, 0.f, 0.f, 0.f), 0, 0); dead++; }
  }
  if (dead) atomicAdd(&T.stats[1], dead);  // tombstones: the key stays (probe chains run through it) until the table is rebuilt
}

// ---------------------------------------------------------------------------------------------- data association
// Largest two eigenvalues + unit eigenvector of the largest, of a symmetric 3x3 (the only outputs LM:500-506 uses of
// Eigen::SelfAdjointEigenSolver).  Closed form (trigonometric solution of the characteristic cubic; eigenvector from the
// best-conditioned cross product of two rows of A - lambda I): ~2 us of dependent f64 latency instead of ~25 us for the
// iterative sweeps the CPU oracle runs.  Agrees with the oracle's Jacobi iteration to ~1e-13 for the well-separated
// spectra of line features; the eigenvector's sign is arbitrary in both.
__device__ void sym_eig3_top(const double A[3][3], double* e_mid, double* e_max, double v[3]) {
  const double q = (A[0][0] + A[1][1] + A[2][2]) / 3.0;
  const double p1 = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
  const double d0 = A[0][0] - q, d1 = A[1][1] - q, d2 = A[2][2] - q;
  const double p2 = d0 * d0 + d1 * d1 + d2 * d2 + 2.0 * p1;
  if (!(p2 > 0.0)) { *e_mid = q; *e_max = q; v[0] = 1; v[1] = 0; v[2] = 0; return; }
  const double p = sqrt(p2 / 6.0), ip = 1.0 / p;
  const double b00 = d0 * ip, b11 = d1 * ip, b22 = d2 * ip, b01 = A[0][1] * ip, b02 = A[0][2] * ip, b12 = A[1][2] * ip;
  double r = 0.5 * (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02));
  r = fmin(1.0, fmax(-1.0, r));
  const double phi = acos(r) / 3.0;
  const double emax = q + 2.0 * p * cos(phi);
  const double emin = q + 2.0 * p * cos(phi + 2.0943951023931954923);  // + 2 pi / 3
  *e_max = emax;
  *e_mid = 3.0 * q - emax - emin;
  const double r0[3] = {A[0][0] - emax, A[0][1], A[0][2]}, r1[3] = {A[0][1], A[1][1] - emax, A[1][2]}, r2[3] = {A[0][2], A[1][2], A[2][2] - emax};
  const double c0[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
  const double c1[3] = {r0[1] * r2[2] - r0[2] * r2[1], r0[2] * r2[0] - r0[0] * r2[2], r0[0] * r2[1] - r0[1] * r2[0]};
  const double c2[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
  const double n0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2], n1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2],
               n2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
  const bool u0 = n0 >= n1 && n0 >= n2, u1 = !u0 && n1 >= n2;
  const double nn = u0 ? n0 : (u1 ? n1 : n2);
  const double inv = 1.0 / sqrt(nn);
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = (u0 ? c0[k] : (u1 ? c1[k] : c2[k])) * inv;
}

// Householder least squares, identical operation order to oracle/orc_math.h householder_ls (m = 5, n = 3; LM:557)
__device__ bool householder_ls_5x3(double* A, double* b, double* x) {
  const int m = 5, n = 3;
  for (int k = 0; k < n; k++) {
    double nrm = 0;
    for (int i = k; i < m; i++) nrm += A[i * n + k] * A[i * n + k];
    nrm = sqrt(nrm);
    if (nrm == 0.0) return false;
    const double alpha = (A[k * n + k] > 0) ? -nrm : nrm;
    const double v0 = A[k * n + k] - alpha;
    double vtv = v0 * v0;
    for (int i = k + 1; i < m; i++) vtv += A[i * n + k] * A[i * n + k];
    if (vtv != 0.0) {
      for (int j = k + 1; j < n; j++) {
        double s = v0 * A[k * n + j];
        for (int i = k + 1; i < m; i++) s += A[i * n + k] * A[i * n + j];
        s = 2.0 * s / vtv;
        A[k * n + j] -= s * v0;
        for (int i = k + 1; i < m; i++) A[i * n + j] -= s * A[i * n + k];
      }
      double s = v0 * b[k];
      for (int i = k + 1; i < m; i++) s += A[i * n + k] * b[i];
      s = 2.0 * s / vtv;
      b[k] -= s * v0;
      for (int i = k + 1; i < m; i++) b[i] -= s * A[i * n + k];
    }
    A[k * n + k] = alpha;
    for (int i = k + 1; i < m; i++) A[i * n + k] = 0.0;
  }
  for (int k = n - 1; k >= 0; k--) {
    double s = b[k];
    for (int j = k + 1; j < n; j++) s -= A[k * n + j] * x[j];
    if (A[k * n + k] == 0.0) return false;
    x[k] = s / A[k * n + k];
  }
  return true;
}

// ---- k_map_assoc: the 5-NN search with G lanes per stack point (G = 16 / 32 / 64; 64 / G queries share a wavefront).
// One query's work is ~27 block probes and ~30 candidate records along a chain of three dependent memory trips: a full wavefront per
// query leaves most lanes idle most of the time and the chip runs out of wave slots, not of bandwidth (round 2: 38 % active, 5 120
// resident waves per 14 us).  Here a group of G lanes walks the same chain for its own query — piece tables by three lanes, one block
// per lane and trip, up to four candidate records per lane in flight — and the best five are taken by five group arg-min rounds over
// the (d2, tie) keys through DPP row operations (keys are unique: distinct voxels), so no candidate list is ranked in LDS any more.
// Results do not depend on G: the keys, not the visiting order, decide.
// amdgpu_waves_per_eu(5): the 16-lane form would take 108 VGPRs (4 wavefronts per SIMD); held to 96 it spills nothing and runs 5
// (B = 8: 101 -> 85 us per launch; 6 wavefronts / 80 VGPRs spills 16 values and loses again: 106 us).  The 32 / 64-lane forms use 80 anyway.
template <int G, int KB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_map_assoc(const float4* __restrict__ stack0, const float4* __restrict__ stack1, VoxelTable T0,
                                                   VoxelTable T1, float inv0, float inv1, const MapState* __restrict__ ms, MapFrame* fr,
                                                   float4* __restrict__ nbr, int outer, int4* __restrict__ cbox, float4* __restrict__ ccand,
                                                   long long* __restrict__ dbg_cyc /* [16] phase cycle sums + wavefront count, or null */, size_t ss) {
  VL_SESSION(ss); RB(stack0); RB(stack1); T0.rebase(so_); T1.rebase(so_); RB(ms); RB(fr); RB(nbr); RB(cbox); RB(ccand); RB(dbg_cyc);
  long long tp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (dbg_cyc) tp[0] = clock64();
  constexpr int Q = 64 / G, QW = 4 * Q;     // queries per wavefront / per workgroup
  constexpr int U = G == 16 ? 4 : 2, CH = U * G;   // candidates per lane and pass / per query and pass (64 / 64 / 128: the typical query has ~30; four per lane in the
  // 32-lane form — one pass for the ~100 candidates of a corner query in a dense map — measured: 96 VGPRs with 13 spills, 23.3 instead of 20.3 us)
  // KB: blocks per lane and trip
  static_assert(CH <= kCandCache, "the second round's candidate cache holds kCandCache entries per slot");   // (rows of CH entries: a query's candidates sit in 1 - 2 KB, not in a 4 KB page of their own)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane & (G - 1), qi = wave * Q + lane / G;
  const int nc = ms->n_corner_stack, nsf = ms->n_surf_stack;
  // XCD-aware assignment as before, in units of QW queries: workgroup b runs on XCD b % 8 and every XCD takes a contiguous eighth of
  // the corner points and a contiguous eighth of the surf points (VoxelGrid output is spatially sorted: neighbours share an L2)
  const int wc = (nc + QW - 1) / QW, ws = (nsf + QW - 1) / QW, cpc = (wc + 7) >> 3, cps = (ws + 7) >> 3;
  const int bq = (int)blockIdx.x >> 3, xcd = (int)blockIdx.x & 7;
  if (bq >= cpc + cps || !ms->do_optimize) return;
  const int kind = bq < cpc ? 0 : 1;        // a workgroup serves one kind
  const int i = (kind ? xcd * cps + (bq - cpc) : xcd * cpc + bq) * QW + qi;
  const bool live = i < (kind ? nsf : nc);
  if (__ballot(live) == 0ull) return;
  const int slot = kind ? kStackCapCorner + i : i;
  const VoxelTable T = kind ? T1 : T0;
  const float inv = kind ? inv1 : inv0;
  const unsigned nv = (unsigned)vox_radix(inv);
  __shared__ u64 s_cand[QW][CH + 8];        // voxel keys of the pass, flattened per query
  __shared__ u64 s_bestk[QW][8];            // the best five so far: key ...
  __shared__ float4 s_bestp[QW][8];         // ... and centroid
  __shared__ int s_piece[QW][3][8];         // per axis: (cube, 4-voxel block, 4-bit mask) pieces of the search range
  __shared__ int s_np[QW][4];               // pieces per axis | overflow flag
  constexpr int kRawCap = 64;
  __shared__ u64 s_rawk[QW][kRawCap];       // raw voxels among the candidates (key, point count): expanded in extra passes
  __shared__ int s_rawn[QW][kRawCap];
  __shared__ int s_nraw[QW];
  float4 pointOri = make_float4(0.f, 0.f, 0.f, 0.f);
  // second outer round: the box of the first round is requested WITH the point and the pose (its address depends on the slot only).  The
  // cache entries are not: fetching the first 2 G of them up front as well was measured (A/B builds) — no change in the launch's duration
  // (10.1 us either way), 4 MB more traffic per sweep for entries beyond the lists' ends.
  int4 box0 = make_int4(0, 0, 0, 0), box1 = make_int4(0, 0, -1, 0);
  if (live) {
    pointOri = kind ? stack1[i] : stack0[i];
    if (outer > 0) { box0 = cbox[2 * slot]; box1 = cbox[2 * slot + 1]; }
  }
  const float4 sel = associate_to_map(pointOri, ms->parameters, ms->parameters + 4);  // LM:476 / LM:542
  const float q0 = sel.x, q1 = sel.y, q2 = sel.z;
  const int cen0 = ms->cenW, cen1 = ms->cenH, cen2 = ms->cenD;
  const int ctr0 = ms->centerCube[0] - cen0, ctr1 = ms->centerCube[1] - cen1, ctr2 = ms->centerCube[2] - cen2;  // absolute centre cube
  // voxel-index box that can hold a point within 1 m (pointSearchSqDis[4] < 1.0 gates everything, LM:479 / LM:547)
  // The FIRST round searches 5 cm more than the 1.001 m it needs: the second round's query — the same point under a pose that moved by
  // millimetres to centimetres — then still finds its box INSIDE the cached one and re-ranks the cached candidates (a superset of its own:
  // the five nearest within 1 m are the same).  With the exact box 15 % of the second round's queries saw a voxel boundary move and
  // searched again, and the launch lasted as long as the slowest of them.
  const float mg = outer == 0 ? 1.051f : 1.001f;
  int blo0 = (int)floorf((q0 - mg) * inv), bhi0 = (int)floorf((q0 + mg) * inv);
  int blo1 = (int)floorf((q1 - mg) * inv), bhi1 = (int)floorf((q1 + mg) * inv);
  int blo2 = (int)floorf((q2 - mg) * inv), bhi2 = (int)floorf((q2 + mg) * inv);
  // second outer round: same box as the first round => same candidates, re-ranked from the cache without a hash probe
  bool from_cache = false;
  int total = 0;
  if (outer > 0 && live) {
    const int4 b0 = box0, b1 = box1;
    from_cache = b1.z >= 0 && b1.z <= kCandCache && b0.x <= blo0 && b0.y >= bhi0 && b0.z <= blo1 && b0.w >= bhi1 && b1.x <= blo2 && b1.y >= bhi2;
    if (from_cache) total = b1.z;
  }
  const bool search = live && !from_cache;
  bool chain_too_long = false;
  if (dbg_cyc) tp[1] = clock64() + (__float_as_int(q0) & 0) + (total & 0);   // (the stamp waits for the loads above)
  if (gl < 8) s_bestk[qi][gl] = ~0ull;
  if (gl < 4) s_np[qi][gl] = 0;
  if (gl == 4) s_nraw[qi] = 0;
  sw_lds_sync();
  if (__ballot(search) != 0ull) {
    // per axis the index range [lo, hi] is cut into (cube, 4-voxel block) pieces — a voxel that straddles a 50 m cube face exists once
    // per cube — each with the 4-bit mask of its voxels inside the range; lane a of the group lists axis a
    if (search && gl < 3) {
      const int lo = gl == 0 ? blo0 : (gl == 1 ? blo1 : blo2), hi = gl == 0 ? bhi0 : (gl == 1 ? bhi1 : bhi2);
      const int ctr = gl == 0 ? ctr0 : (gl == 1 ? ctr1 : ctr2), cen = gl == 0 ? cen0 : (gl == 1 ? cen1 : cen2);
      const int halfw = gl == 2 ? 1 : 2, wdim = gl == 0 ? kCubeW : (gl == 1 ? kCubeH : kCubeD);   // valid block: 5 x 5 x 3 cubes (LM:404-420)
      const double leaf = 1.0 / (double)inv;
      const int Amin = cube_lo((double)lo * leaf), Amax = cube_hi((double)(hi + 1) * leaf);
      int n = 0;
      bool ovf = false;
      for (int A = Amin; A <= Amax; A++) {
        if (abs(A - ctr) > halfw) continue;
        const int wv = A + cen;
        if (wv < 0 || wv >= wdim) continue;
        // voxels that can hold points of cube A: from the voxel containing its lower face to the one containing its upper face
        const int base = cube_voxel_base(A, inv);
        const int ia = max(lo, base + 1), ib = min(hi, cube_voxel_base(A + 1, inv) + 1);
        if (ia > ib) continue;
        for (int blk = (ia - base) >> 2; blk <= ((ib - base) >> 2); blk++) {
          if ((unsigned)blk > (unsigned)(kVoxMax >> 2) || n >= 8) { ovf = true; break; }  // not reachable for the leaves vloam_create accepts (>= 0.132 m: <= 17 voxels = 6 blocks + a cube face)
          int m4 = 0;
#pragma unroll
          for (int t = 0; t < 4; t++) { const int iv = base + (blk << 2) + t; if (iv >= ia && iv <= ib) m4 |= 1 << t; }
          s_piece[qi][gl][n] = ((A + 8192) << 11) | (blk << 4) | m4;
          n++;
        }
      }
      s_np[qi][gl] = n;
      if (ovf) s_np[qi][3] = 1;
    }
    sw_lds_sync();
  }
  const int np0 = s_np[qi][0], np1 = s_np[qi][1], np2 = s_np[qi][2];
  const bool overflow = s_np[qi][3] != 0;
  if (dbg_cyc) tp[2] = clock64() + (np0 & 0);
  const int nblocks = search ? np0 * np1 * np2 : 0;
  // ---- the pieces every pass shares
  u64 key_u[U + 1];                       // (d2, tie) of this lane's candidates of the pass (+ one carried best)
  float px[U + 1], py[U + 1], pz[U + 1];
  int c0 = 0, ncand = 0;                  // pass window [c0, c0 + CH) of the query's candidate ordinals; candidates of this pass
  bool cache_pass = false;                // first-round pass whose candidates are left for the second round
  // phase 3: up to U voxel records per lane, two in flight per trip (the second pair is only touched when some query of the wavefront has
  // more than 2 G candidates); centroid out of the record, squared distance, key = (f32 d2 bits, position of the voxel in the
  // reference's gathered map cloud): laserCloud*FromMap concatenates the valid cubes in (i, j, k) loop order (LM:404-430) and every cube
  // cloud is VoxelGrid output, i.e. sorted by (iz, iy, ix) — so equal distances resolve to the lowest index of that cloud, the oracle's
  // canonical kNN tie rule.  A RAW voxel (points that arrived while its cube was outside the valid block, k_map_finalize) is no
  // candidate itself: it goes onto the query's raw list and its points are looked at one by one in extra passes below.
  auto probe_pair = [&](auto UB) {
    constexpr int u0 = decltype(UB)::value;
    u64 ck[2];
    unsigned sl[2];
    RecVal rv[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int w = gl + (u0 + h) * G;
      ck[h] = w < ncand ? s_cand[qi][w] : 0ull;
      sl[h] = (unsigned)mix64(ck[h]) & T.mask;
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      rv[h].key = 0ull; rv[h].sum = make_float4(0.f, 0.f, 0.f, 0.f); rv[h].count = 0; rv[h].pend_cnt = 0;
      if (gl + (u0 + h) * G < ncand) rv[h] = rec_load(&T.rec[sl[h]]);
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int u = u0 + h;
      if (gl + u * G < ncand) {
        const u64 key = ck[h];
#pragma nounroll
        for (int probe = 0;;) {
          if (rv[h].key == 0ull) break;
          if (rv[h].key == key) {
            const int n = rec_n(rv[h].count);
            const bool raw = rec_raw(rv[h].count);
            float4 p = rv[h].sum;
            if (raw && n >= 2) {   // (a raw voxel of one point IS that point)
              const int pos = atomicAdd(&s_nraw[qi], 1);
              if (pos < kRawCap) { s_rawk[qi][pos] = key; s_rawn[qi][pos] = min(n, 255); }
            } else if (n > 0) {
              if (n > 1) { const float nn = (float)n; p.x = p.x / nn; p.y = p.y / nn; p.z = p.z / nn; }
              const float d0 = q0 - p.x, d1 = q1 - p.y, d2 = q2 - p.z;
              int Ai, Aj, Ak;
              unpack_cube(key, &Ai, &Aj, &Ak);
              // position in the gathered cloud as a mixed-radix number: cube (i, j, k loop order of the 5 x 5 x 3 block) then (lz, ly, lx);
              // every partial result stays below 2^24 until the last step (three full-rate 24-bit multiply-adds)
              const unsigned cube = (unsigned)((Ai - ctr0 + 2) * 15 + (Aj - ctr1 + 2) * 3 + (Ak - ctr2 + 1));
              unsigned tie = ((cube * nv + (unsigned)key_lz(key)) * nv + (unsigned)key_ly(key)) * nv + (unsigned)key_lx(key);
              const int seq = key_seq(key);
              if (seq) { const unsigned nv3 = nv * nv * nv; tie = cube * nv3 + (tie * 2654435761u + (unsigned)seq * 40503u) % nv3; }   // raw points of one voxel: distinct ties inside the cube
              key_u[u] = ((u64)__float_as_uint(d0 * d0 + d1 * d1 + d2 * d2) << 32) | tie;
              px[u] = p.x; py[u] = p.y; pz[u] = p.z;
            }
            break;
          }
          if (++probe == kMaxProbe) { chain_too_long = true; break; }
          sl[h] = (sl[h] + 1) & T.mask;
          rv[h] = rec_load(&T.rec[sl[h]]);
        }
        if (cache_pass)   // leave the candidate for the second round
          ccand[(size_t)slot * kCandCache + c0 + gl + u * G] = make_float4(px[u], py[u], pz[u], __uint_as_float(key_u[u] == ~0ull ? 0xffffffffu : (unsigned)key_u[u]));
      }
    }
  };
  // phase 4: five group arg-min rounds over this pass's candidates (and, with `carry`, the best five of the earlier passes); the
  // winner's lane publishes its centroid and retires the candidate
  auto select_rounds = [&](bool act, bool carry) {
    if (carry && act && gl < 5) {
      key_u[U] = s_bestk[qi][gl];
      const float4 bp = s_bestp[qi][gl];
      px[U] = bp.x; py[U] = bp.y; pz[U] = bp.z;
    }
    sw_lds_sync();
#pragma unroll
    for (int r = 0; r < 5; r++) {
      u64 m = key_u[0];
#pragma unroll
      for (int u = 1; u <= U; u++) m = key_u[u] < m ? key_u[u] : m;
      const u64 gm = grp_min_u64<G>(m);
      if (gm != ~0ull) {
#pragma unroll
        for (int u = 0; u <= U; u++)
          if (key_u[u] == gm) { s_bestk[qi][r] = gm; s_bestp[qi][r] = make_float4(px[u], py[u], pz[u], 0.f); key_u[u] = ~0ull; }
      } else if (act && gl == 0) s_bestk[qi][r] = ~0ull;
    }
    sw_lds_sync();
  };
  auto reset_candidates = [&]() {
#pragma unroll
    for (int u = 0; u <= U; u++) { key_u[u] = ~0ull; px[u] = 0.f; py[u] = 0.f; pz[u] = 0.f; }
  };
  // Candidate lists longer than CH (a dense map at a fine leaf: up to 9^3 voxels in the box) take several passes: every pass regenerates
  // the work list, keeps ordinals [c0, c0 + CH), and the best five so far compete again.
  for (c0 = 0;; c0 += CH) {
    const bool act = live && (c0 == 0 || c0 < total);
    if (__ballot(act) == 0ull) break;
    reset_candidates();
    const bool gen = act && search;
    ncand = 0;
    if (__ballot(gen) != 0ull) {
      // phase 1 + 2: one block per lane and trip fetches its occupancy mask; the existing voxels are flattened into the query's list
      int produced = 0;
      for (int bb0 = 0; __ballot(gen && bb0 < nblocks) != 0ull; bb0 += KB * G) {
        u64 occ[KB], bkey[KB];
        unsigned bs[KB];
        ulonglong2 e[KB];
        int pA[KB][3];   // cube of the block per axis
        int pb[KB][3];   // block index per axis
        int pm[KB][3];   // voxel mask per axis
        bool has[KB];
#pragma unroll
        for (int k = 0; k < KB; k++) {
          const int bb = bb0 + k * G + gl;
          has[k] = gen && bb < nblocks;
          occ[k] = 0ull; bkey[k] = 0ull; bs[k] = 0u;
#pragma unroll
          for (int a = 0; a < 3; a++) { pA[k][a] = 0; pb[k][a] = 0; pm[k][a] = 0; }
          if (has[k]) {
            // bb -> (ex, ey, ez), bb < 512 and np <= 8: quotients through an f32 reciprocal ((bb + 0.5) / n is at least 0.5 / 64 away from
            // an integer, the reciprocal is good to 1 ulp) instead of two ~35-instruction integer divisions
            const int n01 = np0 * np1;
            const int ez = (int)(((float)bb + 0.5f) * __builtin_amdgcn_rcpf((float)n01)), rem = bb - ez * n01;
            const int ey = (int)(((float)rem + 0.5f) * __builtin_amdgcn_rcpf((float)np0)), ex = rem - ey * np0;
            const int w0 = s_piece[qi][0][ex], w1 = s_piece[qi][1][ey], w2 = s_piece[qi][2][ez];
            pA[k][0] = (w0 >> 11) - 8192; pb[k][0] = (w0 >> 4) & 127; pm[k][0] = w0 & 15;
            pA[k][1] = (w1 >> 11) - 8192; pb[k][1] = (w1 >> 4) & 127; pm[k][1] = w1 & 15;
            pA[k][2] = (w2 >> 11) - 8192; pb[k][2] = (w2 >> 4) & 127; pm[k][2] = w2 & 15;
            bkey[k] = pack_key(pA[k][0], pA[k][1], pA[k][2], pb[k][0], pb[k][1], pb[k][2]) | (1ull << 63);
            bs[k] = (unsigned)mix64(bkey[k]) & T.bslots_mask;
          }
        }
#pragma unroll
        for (int k = 0; k < KB; k++) if (has[k]) e[k] = T.blk[bs[k]];   // all first probes in flight together
#pragma unroll
        for (int k = 0; k < KB; k++) {
          if (has[k]) {
#pragma nounroll
            for (int probe = 0;;) {   // (collisions are rare: keep the chain walk a compact loop)
              if (e[k].x == 0ull) break;
              if (e[k].x == bkey[k]) { occ[k] = e[k].y; break; }
              if (++probe == kMaxProbe) { chain_too_long = true; break; }
              bs[k] = (bs[k] + 1) & T.bslots_mask;
              e[k] = T.blk[bs[k]];
            }
            // voxels of the block inside the search box: bit = z * 16 + y * 4 + x
            const int mx = pm[k][0], my = pm[k][1], mz = pm[k][2];
            const u64 ex4 = (u64)mx * 0x1111111111111111ull;
            const u64 ey4 = ((u64)((my & 1) * 0xF) | ((u64)(((my >> 1) & 1) * 0xF) << 4) | ((u64)(((my >> 2) & 1) * 0xF) << 8) | ((u64)(((my >> 3) & 1) * 0xF) << 12)) * 0x0001000100010001ull;
            const u64 ez4 = ((mz & 1) ? 0xFFFFull : 0ull) | ((mz & 2) ? 0xFFFFull << 16 : 0ull) | ((mz & 4) ? 0xFFFFull << 32 : 0ull) | ((mz & 8) ? 0xFFFFull << 48 : 0ull);
            occ[k] &= ex4 & ey4 & ez4;
          }
        }
#pragma unroll
        for (int k = 0; k < KB; k++) {
          // flatten: exclusive prefix of the per-lane voxel counts inside the group, then every lane appends its voxel keys
          const int mine = __popcll(occ[k]);
          const int inc = grp_scan_incl<G>(mine);
          const int tot = grp_sum<G>(mine);
          int o = produced + inc - mine;
          u64 oc = occ[k];
          while (oc) {
            const int bit = __ffsll((long long)oc) - 1;
            oc &= oc - 1;
            if (o >= c0 && o < c0 + CH)
              s_cand[qi][o - c0] = pack_key(pA[k][0], pA[k][1], pA[k][2], (pb[k][0] << 2) | (bit & 3), (pb[k][1] << 2) | ((bit >> 2) & 3), (pb[k][2] << 2) | (bit >> 4));
            o++;
          }
          produced += tot;
        }
      }
      if (gen) total = produced;
      sw_lds_sync();
      ncand = gen ? min(total - c0, CH) : 0;
      if (dbg_cyc && c0 == 0) tp[3] = clock64() + (ncand & 0);
      cache_pass = outer == 0 && total <= kCandCache;   // (lists of up to kCandCache candidates: every pass leaves its part)
      probe_pair(std::integral_constant<int, 0>{});
      if constexpr (U > 2) { if (__ballot(2 * G < ncand) != 0ull) probe_pair(std::integral_constant<int, 2>{}); }
      cache_pass = false;
    }
    if (__ballot(from_cache && act) != 0ull) {
      // all of a lane's cache entries of the pass in flight together, complete 16-byte entries (a load that is conditional on the entry's own
      // tie field turns into two dependent trips per entry)
      float4 cc[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int w = c0 + gl + u * G;
        cc[u] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xffffffffu));
        if (from_cache && act && w < total) cc[u] = ccand[(size_t)slot * kCandCache + w];
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const unsigned tie = __float_as_uint(cc[u].w);
        const float d0 = q0 - cc[u].x, d1 = q1 - cc[u].y, d2 = q2 - cc[u].z;
        const u64 k = ((u64)__float_as_uint(d0 * d0 + d1 * d1 + d2 * d2) << 32) | tie;
        if (from_cache && tie != 0xffffffffu) { key_u[u] = k; px[u] = cc[u].x; py[u] = cc[u].y; pz[u] = cc[u].z; }
      }
    }
    if (dbg_cyc && c0 == 0) tp[4] = clock64() + ((int)key_u[0] & 0);
    select_rounds(act, c0 > 0);
    if (dbg_cyc && c0 == 0) tp[5] = clock64();
  }
  // ---- raw voxels among the candidates (only with returns beyond the valid block, i.e. ranges over 100 m): their points, one record each
  // (seq 1..n), go through the same probe + arg-min passes, the best five so far carried along
  const int nraw = min(s_nraw[qi], kRawCap);
  const bool raw_overflow = s_nraw[qi] > kRawCap;
  if (__ballot(live && nraw > 0) != 0ull) {
    int total_raw = 0;
    for (c0 = 0;; c0 += CH) {
      const bool act = live && nraw > 0 && (c0 == 0 || c0 < total_raw);
      if (__ballot(act) == 0ull) break;
      reset_candidates();
      int produced = 0;
      for (int r0 = 0; __ballot(act && r0 < nraw) != 0ull; r0 += G) {
        const int r = r0 + gl;
        const int nr = (act && r < nraw) ? s_rawn[qi][r] : 0;
        const u64 vk = (act && r < nraw) ? s_rawk[qi][r] : 0ull;
        const int inc = grp_scan_incl<G>(nr);
        const int tot = grp_sum<G>(nr);
        int o = produced + inc - nr;
        for (int j = 1; j <= nr; j++, o++)
          if (o >= c0 && o < c0 + CH) s_cand[qi][o - c0] = key_with_seq(vk, j);
        produced += tot;
      }
      if (act) total_raw = produced;
      sw_lds_sync();
      ncand = act ? min(total_raw - c0, CH) : 0;
      probe_pair(std::integral_constant<int, 0>{});
      if constexpr (U > 2) { if (__ballot(2 * G < ncand) != 0ull) probe_pair(std::integral_constant<int, 2>{}); }
      select_rounds(act, true);
    }
  }
  if (outer == 0 && search && gl == 0) {
    cbox[2 * slot] = make_int4(blo0, bhi0, blo1, bhi1);
    cbox[2 * slot + 1] = make_int4(blo2, bhi2, (total <= kCandCache && !overflow && s_nraw[qi] == 0) ? total : -1, total);   // (.w: the count itself, tools/assoc_phases.py)
  }
  // hand the five neighbours to k_map_fit (one THREAD per query there: the 3x3 eigen / 5x3 least-squares fits are heavy in registers
  // and pure per-query math) — as points, so that the fit does not have to go back to the table
  if (live && gl < 5) {
    const u64 k4 = s_bestk[qi][4];
    const bool ok = k4 != ~0ull && __uint_as_float((unsigned)(k4 >> 32)) < 1.0f;  // LM:479 / LM:547
    float4 p = s_bestp[qi][gl];
    p.w = ok ? 1.0f : 0.0f;
    nbr[slot * 5 + gl] = p;
  }
  if (live && gl == 0 && total > kCandChunk) atomicMax(&fr->max_candidates, total);
  if (__ballot(chain_too_long || (live && overflow)) && lane == 0) atomicOr(&fr->error, kErrMapFull);
  if (__ballot(live && raw_overflow) && lane == 0) atomicOr(&fr->error, kErrMapDeferred);
  if (dbg_cyc && lane == 0) {   // debug builds of the handle: where a wavefront's time goes (setup | pieces | blocks + flatten | records | arg-min rounds)
    tp[6] = clock64();
    if (tp[3] == 0) tp[3] = tp[2];
    if (tp[4] == 0) tp[4] = tp[3];
    for (int k = 0; k < 6; k++) atomicAdd((unsigned long long*)&dbg_cyc[outer * 8 + k], (unsigned long long)(tp[k + 1] - tp[k]));
    atomicAdd((unsigned long long*)&dbg_cyc[outer * 8 + 7], 1ull);
  }
}

// k_map_prepare / k_map_fit in their two forms (the include file takes its five parameters as macros and undefines them at its end)
#define VL_MAP_TIER 0
#define VL_MAP_KERNEL(name) name
#define VL_MAP_CAP_PARAM
#define VL_MAP_SURF_CAP kStackCapSurf
#define VL_MAP_FACTOR_CAP kMapFactorCap
#include "map_prepare_fit.inc.h"
#define VL_MAP_TIER 1
#define VL_MAP_KERNEL(name) name##_tier
#define VL_MAP_CAP_PARAM , int surf_cap
#define VL_MAP_SURF_CAP surf_cap
#define VL_MAP_FACTOR_CAP F.cap
#include "map_prepare_fit.inc.h"

// ---------------------------------------------------------------------------------------------- update / insert / finalize
// transformUpdate + the map half of the trajectory row; done by one lane of k_map_insert (nothing else in that launch reads
// q_wmap_wodom / t_wmap_wodom)
__device__ void map_update(MapState* ms, double* traj_row14) {
  // transformUpdate LM:140-144: q_wmap_wodom = q_w_curr * q_wodom_curr^-1 ; t_wmap_wodom = t_w_curr - q_wmap_wodom * t_wodom_curr
  const double* q = ms->q_wodom_curr;
  const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  double qi[4] = {0, 0, 0, 0};
  if (n2 > 0.0) { qi[0] = -q[0] / n2; qi[1] = -q[1] / n2; qi[2] = -q[2] / n2; qi[3] = q[3] / n2; }
  double r[4], t[3];
  dquat_mul(ms->parameters, qi, r);
  for (int k = 0; k < 4; k++) ms->q_wmap_wodom[k] = r[k];
  dquat_rot(ms->q_wmap_wodom, ms->t_wodom_curr, t);
  for (int k = 0; k < 3; k++) ms->t_wmap_wodom[k] = ms->parameters[4 + k] - t[k];
  if (traj_row14) for (int k = 0; k < 7; k++) traj_row14[7 + k] = ms->parameters[k];
}

// One raw point of a voxel as a record of its own: key | seq, sum = the point, count = 1, pend_cnt = arrival stamp (sweep << 14 | stack
// index — sweep << 17 | stack index on a handle of the large stack tier, k_map_finalize; 0 for a centroid that became raw point number one).  find-or-insert: a purged record of the same key is reused.
__device__ bool map_put_raw_point(const VoxelTable& T, u64 voxel_key, int seq, float4 p, int stamp) {
  const u64 key = key_with_seq(voxel_key, seq);
  unsigned s = (unsigned)mix64(key) & T.mask;
  for (int probe = 0; probe < kMaxProbe; probe++, s = (s + 1) & T.mask) {
    const u64 old = atomicCAS(&T.rec[s].key, 0ull, key);
    if (old == 0ull || old == key) {
      if (old == 0ull) atomicAdd(&T.stats[0], 1);
      rec_store_value(&T.rec[s], p, 1, stamp);
      return true;
    }
  }
  return false;
}
// the cube is valid again: the raw points of the voxel are merged into its centroid and their records retire (key kept, count 0: purged)
__device__ void map_drop_raw_points(const VoxelTable& T, u64 voxel_key, int n) {
  int dead = 0;
  for (int seq = 1; seq <= min(n, 255); seq++) {
    const u64 key = key_with_seq(voxel_key, seq);
    unsigned s = (unsigned)mix64(key) & T.mask;
    for (int probe = 0; probe < kMaxProbe; probe++, s = (s + 1) & T.mask) {
      const u64 k = T.rec[s].key;
      if (k == 0ull) break;
      if (k == key) { rec_store_value(&T.rec[s], make_float4(0.f, 0.f, 0.f, 0.f), 0, 0); dead++; break; }
    }
  }
  if (dead) atomicAdd(&T.stats[1], dead);
}

template <bool TIER>
__device__ __forceinline__ void map_insert_body(const float4* __restrict__ stack0, const float4* __restrict__ stack1,
                                                float4* __restrict__ smap0, float4* __restrict__ smap1, VoxelTable T0, VoxelTable T1,
                                                float inv0, float inv1, MapState* ms, MapFrame* fr, int* __restrict__ touched0,
                                                int* __restrict__ touched1, int* __restrict__ deferred0, int* __restrict__ deferred1,
                                                double* traj_row14, size_t ss, int surf_cap) {
  VL_SESSION(ss); RB(stack0); RB(stack1); RB(smap0); RB(smap1); T0.rebase(so_); T1.rebase(so_); RB(ms); RB(fr); RB(touched0); RB(touched1);
  RB(deferred0); RB(deferred1); RB(traj_row14);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) map_update(ms, traj_row14);  // LM:636
  const int kind = blockIdx.y;
  const VoxelTable T = kind ? T1 : T0;
  const float inv = kind ? inv1 : inv0;
  const float4* stack = kind ? stack1 : stack0;
  float4* smap = kind ? smap1 : smap0;
  int* touched = kind ? touched1 : touched0;
  (void)deferred0; (void)deferred1;
  const int n = kind ? ms->n_surf_stack : ms->n_corner_stack;
  const int cap = kind ? (TIER ? surf_cap : kStackCapSurf) : kStackCapCorner;
  const int lane = threadIdx.x & 63;
  // the thread's first stack point is requested together with the stack size, not behind it (the stale tail of the array is valid memory)
  const int i_first = blockIdx.x * 256 + threadIdx.x;
  const float4 p_first = stack[i_first < cap ? i_first : 0];
  for (int i0 = blockIdx.x * 256 + (threadIdx.x & ~63); i0 < n; i0 += gridDim.x * 256) {   // wavefront-uniform
    const int i = i0 + lane;
    // returns the slot if this point is the first of the sweep in its voxel (the voxel joins the touched list), else -1
    auto insert_point = [&]() -> int {
      if (i >= n) return -1;
      const float4 p = associate_to_map(i == i_first ? p_first : stack[i], ms->parameters, ms->parameters + 4);  // LM:641 / LM:664
      smap[i] = p;
      const int Ai = cube_abs((double)p.x), Aj = cube_abs((double)p.y), Ak = cube_abs((double)p.z);
      const int wi = Ai + ms->cenW, wj = Aj + ms->cenH, wk = Ak + ms->cenD;  // == cubeI, cubeJ, cubeK of LM:643-652
      if (wi < 0 || wi >= kCubeW || wj < 0 || wj >= kCubeH || wk < 0 || wk >= kCubeD) return -1;  // LM:654-655: outside the grid -> dropped
      const int lx = (int)floorf(p.x * inv) - cube_voxel_base(Ai, inv), ly = (int)floorf(p.y * inv) - cube_voxel_base(Aj, inv),
                lz = (int)floorf(p.z * inv) - cube_voxel_base(Ak, inv);
      if ((unsigned)lx > (unsigned)kVoxMax || (unsigned)ly > (unsigned)kVoxMax || (unsigned)lz > (unsigned)kVoxMax || !cube_in_key_range(Ai, Aj, Ak)) { atomicOr(&fr->error, kErrMapFull); return -1; }
      const u64 key = pack_key(Ai, Aj, Ak, lx, ly, lz);
      unsigned s = (unsigned)mix64(key) & T.mask;
      for (int probe = 0; probe < kMaxProbe; probe++, s = (s + 1) & T.mask) {
        const u64 old = atomicCAS(&T.rec[s].key, 0ull, key);
        if (old == 0ull || old == key) {
          if (old == 0ull) {  // new voxel: publish it in its block's occupancy mask
            atomicAdd(&T.stats[0], 1);
            if (!map_publish_block(T, Ai, Aj, Ak, lx, ly, lz)) atomicOr(&fr->error, kErrMapFull);
          }
          const int pos = atomicAdd(&T.rec[s].pend_cnt, 1);
          if (pos < kPendCap) T.pend[(size_t)s * kPendCap + pos] = i; else atomicOr(&fr->error, kErrMapFull);
          return pos == 0 ? (int)s : -1;   // (whether the cube is inside the valid block is k_map_finalize's business: raw points, see there)
        }
      }
      atomicOr(&fr->error, kErrMapFull);
      return -1;
    };
    const int first = insert_point();
    // touched list: one counter update per wavefront instead of one per voxel on the same word
    const u64 tm = __ballot(first >= 0);
    if (tm != 0ull) {
      const int leader = __ffsll((long long)tm) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(&fr->n_touched[kind], __popcll(tm));
      base = __shfl(base, leader);
      if (first >= 0) {
        const int tpos = base + __popcll(tm & ((1ull << lane) - 1ull));
        if (tpos < cap) touched[tpos] = first; else atomicOr(&fr->error, kErrMapFull);
      }
    }
  }
}
#define VL_MAP_INSERT_PARAMS const float4* __restrict__ stack0, const float4* __restrict__ stack1, float4* __restrict__ smap0, float4* __restrict__ smap1, \
    VoxelTable T0, VoxelTable T1, float inv0, float inv1, MapState* ms, MapFrame* fr, int* __restrict__ touched0, int* __restrict__ touched1,      \
    int* __restrict__ deferred0, int* __restrict__ deferred1, double* traj_row14, size_t ss
#define VL_MAP_INSERT_ARGS stack0, stack1, smap0, smap1, T0, T1, inv0, inv1, ms, fr, touched0, touched1, deferred0, deferred1, traj_row14, ss
__global__ __launch_bounds__(256) void k_map_insert(VL_MAP_INSERT_PARAMS) { map_insert_body<false>(VL_MAP_INSERT_ARGS, kStackCapSurf); }
__global__ __launch_bounds__(256) void k_map_insert_tier(VL_MAP_INSERT_PARAMS, int surf_cap) { map_insert_body<true>(VL_MAP_INSERT_ARGS, surf_cap); }
#undef VL_MAP_INSERT_PARAMS
#undef VL_MAP_INSERT_ARGS

template <bool TIER>
__device__ __forceinline__ void map_finalize_body(const float4* __restrict__ smap0, const float4* __restrict__ smap1, VoxelTable T0,
                                                  VoxelTable T1, MapState* ms, MapFrame* fr,
                                                  const int* __restrict__ touched0, const int* __restrict__ touched1,
                                                  int* __restrict__ deferred0, int* __restrict__ deferred1, int* __restrict__ newraw0,
                                                  int* __restrict__ newraw1, int* __restrict__ cube_cnt, int* host_flags, long long* ts_log, size_t ss,
                                                  int surf_cap) {
  VL_SESSION(ss); RB(smap0); RB(smap1); T0.rebase(so_); T1.rebase(so_); RB(ms); RB(fr); RB(touched0); RB(touched1); RB(deferred0); RB(deferred1);
  RB(newraw0); RB(newraw1); RB(cube_cnt); RB(ts_log);
  if (ts_log && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ts_log[2 * ((ms->sweep_no - 1) & 1023) + 1] = (long long)wall_clock64();   // START of the sweep's last launch
  if (host_flags) host_flags += 2 * blockIdx.z;   // host-mapped, one pair per session (not part of the arenas)
  const int kind = blockIdx.y;
  const VoxelTable T = kind ? T1 : T0;
  const float4* smap = kind ? smap1 : smap0;
  const int* touched = kind ? touched1 : touched0;
  const int cap = kind ? (TIER ? surf_cap : kStackCapSurf) : kStackCapCorner;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int s_spec = touched[t < cap ? t : 0];   // requested together with the list's length, not behind it (stale entries are valid slots)
  const int nt = min(fr->n_touched[kind], cap);
  const int cI = ms->centerCube[0], cJ = ms->centerCube[1], cK = ms->centerCube[2];
  int* deferred = kind ? deferred1 : deferred0;
  int* newraw = kind ? newraw1 : newraw0;
  if (t < nt) {
    const int s = s_spec;
    int idx[kPendCap];
    const RecVal rv = rec_load(&T.rec[s]);
    const int np = min(rv.pend_cnt, kPendCap);
    for (int a = 0; a < np; a++) idx[a] = T.pend[(size_t)s * kPendCap + a];
    for (int a = 1; a < np; a++) {  // stack order == the order the reference push_back()s into the cube cloud
      const int v = idx[a];
      int c = a - 1;
      while (c >= 0 && idx[c] > v) { idx[c + 1] = idx[c]; c--; }
      idx[c + 1] = v;
    }
    const int n_old = rec_n(rv.count);
    const bool was_raw = rec_raw(rv.count);
    float4 acc = n_old > 0 ? rv.sum : make_float4(0.f, 0.f, 0.f, 0.f);
    int Ai, Aj, Ak;
    unpack_cube(rv.key, &Ai, &Aj, &Ak);
    const int wi = Ai + ms->cenW, wj = Aj + ms->cenH, wk = Ak + ms->cenD;
    int* cube_n = &cube_cnt[kind * kCubeNum + wi + kCubeW * wj + kCubeW * kCubeH * wk];   // points of the cube's cloud (the LM:448 gate counts them)
    const bool valid = abs(wi - cI) <= 2 && abs(wj - cJ) <= 2 && abs(wk - cK) <= 1;
    if (valid) {
      // VoxelGrid re-filter of a valid cube (LM:689-702): centroid of (what the cube held of this voxel — its centroid, or raw points in
      // arrival order —, new points...): the running f32 sum already is that sum in that order
      if (was_raw) map_drop_raw_points(T, rv.key, n_old);
      for (int a = 0; a < np; a++) { const float4 p = smap[idx[a]]; acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w; }
      const float nn = (float)(n_old + np);
      acc.x = acc.x / nn; acc.y = acc.y / nn; acc.z = acc.z / nn; acc.w = acc.w / nn;
      const int held = was_raw ? n_old : (n_old > 0 ? 1 : 0);
      if (held != 1) atomicAdd(cube_n, 1 - held);
      rec_store_value(&T.rec[s], acc, 1, 0);
    } else {
      // The cube is outside the valid block: the reference appends the points to the cube's cloud and leaves them there un-merged until
      // the cube is next valid (LM:654-659 push_back, LM:689 only filters valid cubes) — its kd-tree then sees them one by one.  The
      // seq-0 record keeps the running sum (the eventual centroid), every point also gets a record of its own (seq 1..n: k_map_assoc
      // expands a raw voxel into them, vloam_get_map emits them); an existing centroid becomes raw point number one.
      int seq = n_old;
      bool overflow = false;
      if (!was_raw) {
        if (n_old == 1 && !map_put_raw_point(T, rv.key, 1, rv.sum, 0)) overflow = true;   // stamp 0: belongs to the filtered (voxel-ordered) part
        // (onto a list of its own: workgroup 0 compacts the raw-voxel list in this very launch; k_map_prepare of the next sweep merges)
        const int dpos = atomicAdd(&fr->n_newraw[kind], 1);
        if (dpos < cap) newraw[dpos] = s; else atomicOr(&fr->error, kErrMapFull);   // the list of raw voxels is full: say so
        atomicAdd(&ms->deferred, 1);
      }
      for (int a = 0; a < np; a++) {
        const float4 p = smap[idx[a]];
        acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
        seq++;
        // arrival stamp = (sweep, stack index): the order key of un-merged points in k_map_export.  The default form's 14 index bits date from
        // the 16 384-point stack; the tier form takes 17 (indices up to kStackCapSurfMax - 1) and 15 sweep bits
        const int stamp = TIER ? (int)(((unsigned)ms->sweep_no & 0x7fffu) << 17) | idx[a] : ((ms->sweep_no & 0x3ffff) << 14) | idx[a];
        if (seq > 255 || !map_put_raw_point(T, rv.key, seq, p, stamp)) overflow = true;
      }
      if (overflow) atomicOr(&fr->error, kErrMapDeferred);   // more than 255 raw points in one voxel, or no slot for one
      atomicAdd(cube_n, np);
      rec_store_value(&T.rec[s], acc, min(seq, 0xffff) | kRecRaw, 0);
    }
  }
  // Raw voxels of earlier sweeps whose cube is valid now (only with ranges beyond the 5x5x3 block): the reference's re-filter of the
  // valid cubes (LM:689-702) merges them in the first sweep their cube is valid, touched or not.  One workgroup walks the list,
  // resolves what became valid and COMPACTS the rest in place (chunks of 256, left to right: an entry only ever moves left), so the
  // list holds the currently-raw voxels only.  A slot that also received points this sweep (pend_cnt > 0, or no longer raw) is
  // finalised by its own thread above — with the validity rule applied to the whole sum — and only leaves the list here.
  if (blockIdx.x == 0) {
    __shared__ int s_wcnt[4], s_out;
    const int nd = min(fr->n_deferred[kind], cap);
    if (threadIdx.x == 0) s_out = 0;
    __syncthreads();
    for (int base = 0; base < nd; base += 256) {
      const int d = base + threadIdx.x;
      int s = d < nd ? deferred[d] : -1;
      if (s >= 0) {
        const RecVal dv = rec_load(&T.rec[s]);
        int Ai, Aj, Ak;
        unpack_cube(dv.key, &Ai, &Aj, &Ak);
        const int wi = Ai + ms->cenW, wj = Aj + ms->cenH, wk = Ak + ms->cenD;
        const bool in_window = wi >= 0 && wi < kCubeW && wj >= 0 && wj < kCubeH && wk >= 0 && wk < kCubeD;
        if (!in_window || dv.count == 0) s = -1;   // purged with its cube
        else if (abs(wi - cI) <= 2 && abs(wj - cJ) <= 2 && abs(wk - cK) <= 1) {
          if (dv.pend_cnt == 0 && rec_raw(dv.count)) {
            const int n = rec_n(dv.count);
            map_drop_raw_points(T, dv.key, n);
            float4 a = dv.sum; const float nn = (float)n;
            a.x /= nn; a.y /= nn; a.z /= nn; a.w /= nn;
            rec_store_value(&T.rec[s], a, 1, 0);
            if (n != 1) atomicAdd(&cube_cnt[kind * kCubeNum + wi + kCubeW * wj + kCubeW * kCubeH * wk], 1 - n);
          }
          s = -1;
        }
      }
      const unsigned long long keep = __ballot(s >= 0);
      if ((threadIdx.x & 63) == 0) s_wcnt[threadIdx.x >> 6] = __popcll(keep);
      __syncthreads();   // every entry of the chunk has been read
      int o = s_out;
      for (int w = 0; w < (int)(threadIdx.x >> 6); w++) o += s_wcnt[w];
      if (s >= 0) deferred[o + __popcll(keep & ((1ull << (threadIdx.x & 63)) - 1ull))] = s;
      __syncthreads();
      if (threadIdx.x == 0) s_out += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
      __syncthreads();
    }
    if (threadIdx.x == 0) fr->n_deferred[kind] = s_out;
  }
  if (fr->rolled) map_purge(T, ms, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
  // table health, once per sweep and kind: the error surfaces well before probe chains degrade, and the host learns (through a
  // host-mapped word it polls without synchronising) when enough purged entries have piled up for a rebuild to pay
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const long long slots = (long long)T.mask + 1;
    const int keys = T.stats[0], dead = T.stats[1];
    if ((long long)(keys - dead) * 10 > slots * 6 || (long long)T.stats[2] * 10 > ((long long)T.bslots_mask + 1) * 6) atomicOr(&fr->error, kErrMapFull);
    if (host_flags) {
      const int want = ((long long)dead * 8 > slots || (long long)keys * 2 > slots) && dead > 0 ? 1 : 0;
      __hip_atomic_store(&host_flags[kind], want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
#define VL_MAP_FINALIZE_PARAMS const float4* __restrict__ smap0, const float4* __restrict__ smap1, VoxelTable T0, VoxelTable T1, MapState* ms, MapFrame* fr, \
    const int* __restrict__ touched0, const int* __restrict__ touched1, int* __restrict__ deferred0, int* __restrict__ deferred1,                      \
    int* __restrict__ newraw0, int* __restrict__ newraw1, int* __restrict__ cube_cnt, int* host_flags, long long* ts_log, size_t ss
#define VL_MAP_FINALIZE_ARGS smap0, smap1, T0, T1, ms, fr, touched0, touched1, deferred0, deferred1, newraw0, newraw1, cube_cnt, host_flags, ts_log, ss
__global__ __launch_bounds__(256) void k_map_finalize(VL_MAP_FINALIZE_PARAMS) { map_finalize_body<false>(VL_MAP_FINALIZE_ARGS, kStackCapSurf); }
__global__ __launch_bounds__(256) void k_map_finalize_tier(VL_MAP_FINALIZE_PARAMS, int surf_cap) { map_finalize_body<true>(VL_MAP_FINALIZE_ARGS, surf_cap); }
#undef VL_MAP_FINALIZE_PARAMS
#undef VL_MAP_FINALIZE_ARGS

// ---------------------------------------------------------------------------------------------- table rebuild (tombstone reclamation)
// Purged entries keep their key so that probe chains stay intact; on a long drive they would fill the table.  When the host sees
// the flag k_map_finalize raises, it enqueues — between two sweeps, on the mapping stream — gather (live records -> list), two
// memsets, reinsert (the movers' one text: map_move_dev.h).  Voxel contents are untouched: only slot positions change (nothing keeps slot
// ids across sweeps except the deferred list, which is rebuilt here).
__global__ __launch_bounds__(256) void k_map_rebuild_gather(VoxelTable T, VoxelRec* __restrict__ tmp, int cap, int* n_tmp, MapFrame* fr, int kind) {
  if (blockIdx.x == 0 && threadIdx.x == 0) map_move_begin(T, fr, kind);   // (nothing in this launch reads what it writes)
  for (unsigned s = blockIdx.x * 256 + threadIdx.x; s <= T.mask; s += gridDim.x * 256) {
    const RecVal v = rec_load(&T.rec[s]);
    if (!rec_live(v)) continue;
    const int o = atomicAdd(n_tmp, 1);
    if (o < cap) rec_store_all(&tmp[o], v);
    else atomicOr(&fr->error, kErrMapFull);
  }
}
__global__ __launch_bounds__(256) void k_map_rebuild_insert(VoxelTable T, const VoxelRec* __restrict__ tmp, int cap, int* n_tmp, MapFrame* fr, int kind,
                                                            int* __restrict__ deferred, int deferred_cap, int* host_flags) {
  const int n = min(*n_tmp, cap);
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256)
    map_reinsert(T, rec_load(&tmp[e]), fr, kind, deferred, deferred_cap);   // (the list holds live records only)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    T.stats[0] = n;   // keys in the table (the block keys are counted by map_publish_block)
    if (host_flags) __hip_atomic_store(&host_flags[kind], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---------------------------------------------------------------------------------------------- host side
vloam_status map_layout(MapContext* m, const vloam_config& cfg, Arena& A) {
  bool ok = true;
  ok = ok && A.take(&m->state, 1) && A.take(&m->frame, 1) && A.take(&m->cube_cnt, 2 * (size_t)kCubeNum);
  const int lg = cfg.map_capacity_log2 < 10 ? 10 : (cfg.map_capacity_log2 > 28 ? 28 : cfg.map_capacity_log2);
  const size_t slots = (size_t)1 << lg;
  for (int k = 0; k < 2 && ok; k++) {
    VoxelTable& T = m->tab[k];
    if (m->grow) { T.rec = nullptr; T.pend = nullptr; T.blk = nullptr; ok = ok && A.take(&T.stats, 4); }   // growable: rec / pend / blk are allocations of their own (map_grow_init)
    else ok = ok && A.take(&T.rec, slots) && A.take(&T.pend, slots * kPendCap) && A.take(&T.stats, 4);
    T.mask = (unsigned)(slots - 1);
    const size_t bslots = slots / 2;
    if (!m->grow) ok = ok && A.take(&T.blk, bslots);
    T.bslots_mask = (unsigned)(bslots - 1);
    DsScratch& D = m->ds[k];
    if (k == 0) for (int c = 0; c < MapContext::kSets; c++) ok = ok && A.take(&m->stack_info[c], 1);
    D.stack_cap = k ? m->surf_cap : kStackCapCorner;
    ok = ok && A.take(&D.region, (size_t)kDsMaxBins * kDsBinCap) && A.take(&D.over, (size_t)cfg.max_points) && A.take(&D.tmp, (size_t)cfg.max_points) &&
         A.take(&D.sorted, (size_t)cfg.max_points) && A.take(&D.splitters, (size_t)kDsMaxBins) && A.take(&D.cursor, (size_t)kDsMaxBins + 4) &&
         A.take(&D.done, (size_t)kDsMaxBins);
    for (int c = 0; c < MapContext::kSets; c++) ok = ok && A.take(&m->stack_sets[c][k], (size_t)D.stack_cap);
    m->stack[k] = m->stack_sets[0][k];
    ok = ok && A.take(&m->stack_map[k], (size_t)D.stack_cap) && A.take(&m->touched[k], (size_t)D.stack_cap) && A.take(&m->deferred[k], (size_t)D.stack_cap) &&
         A.take(&m->newraw[k], (size_t)D.stack_cap);
    FactorTable& F = m->F[k];
    F.cap = m->factor_cap();
    ok = ok && A.take(&F.type, (size_t)F.cap) && A.take(&F.p, 3 * (size_t)F.cap) && A.take(&F.A, 3 * (size_t)F.cap) && A.take(&F.B, 3 * (size_t)F.cap) &&
         A.take(&F.resid, 3 * (size_t)F.cap) && A.take(&F.ctype, (size_t)F.cap) && A.take(&F.cslot, (size_t)F.cap) && A.take(&F.cpack, 11 * (size_t)F.cap) && A.take(&F.dg, 8 * (size_t)F.cap) &&
         A.take(&F.rowcnt, (size_t)F.cap / 64 + 1);
    if (m->tier()) F.rowmask = nullptr;   // more than 512 rows: k_map_fit_tier leaves row counts and the solve takes the packed form (lm_launch)
    else ok = ok && A.take(&F.rowmask, (size_t)F.cap / 64 + 2);
    F.gsync = nullptr;  // the handle places the sync words (lm_sync_calibrate)
    F.err = ok ? &m->frame->error : nullptr;
    F.fallbacks = ok ? &m->frame->fallback_solves : nullptr;
    F.host_degraded = nullptr;   // (the handle points it at its host-mapped word)
    F.gen = 0; F.spin_limit = 1 << 18;
  }
  ok = ok && A.take(&m->rec, 2) && A.take(&m->nbr, 5 * (size_t)m->factor_cap());
  ok = ok && A.take(&m->cbox, 2 * (size_t)m->factor_cap()) && A.take(&m->ccand, (size_t)m->factor_cap() * kCandCache);
  m->rebuild_cap = m->grow ? 0 : (int)(slots / 2);
  if (m->grow) { m->rebuild_tmp = nullptr; m->grow->lg[0] = m->grow->lg[1] = lg; ok = ok && A.take(&m->rebuild_n, 2); }   // a growable handle reclaims through k_map_grow: no staging list
  else ok = ok && A.take(&m->rebuild_tmp, (size_t)m->rebuild_cap) && A.take(&m->rebuild_n, 2);
  ok = ok && A.take(&m->registered, (size_t)cfg.max_points) && A.take(&m->assoc_cyc, 16) && A.take(&m->ts_log, 2048);
  MapPub& P = m->pub;   // published clouds: nothing on a handle that did not ask for them
  if (P.pub_number > 0) {
    ok = ok && A.take(&P.cnt, (size_t)kPubBuckets) && A.take(&P.off, (size_t)kPubBuckets + 1) && A.take(&P.cur, (size_t)kPubBuckets) &&
         A.take(&P.keys, (size_t)P.cap) && A.take(&P.vals, (size_t)P.cap);
    for (int k = 0; k < 2; k++) ok = ok && A.take(&P.out[k], (size_t)P.cap) && A.take(&P.hdr[k], 1);
  }
  if (P.cloud_on) for (int k = 0; k < 2; k++) ok = ok && A.take(&P.cloud[k], (size_t)cfg.max_points) && A.take(&P.cloud_n[k], 1);
  if (!ok) return VLOAM_ERR_HIP;
  m->max_points = cfg.max_points;
  m->inv_leaf[0] = 1.0f / cfg.mapping_line_resolution;   // inverse_leaf_size_ of downSizeFilterCorner (LM:100)
  m->inv_leaf[1] = 1.0f / cfg.mapping_plane_resolution;  // downSizeFilterSurf (LM:101)
  return VLOAM_OK;
}

vloam_status map_init(MapContext* m, hipStream_t st) {
  if (m->grow && map_grow_init(m, st) != VLOAM_OK) return VLOAM_ERR_HIP;
  if (!m->host_flags) {
    if (hipHostMalloc((void**)&m->host_flags, sizeof(int) * 2 * kMaxBatch, hipHostMallocMapped) != hipSuccess) { m->host_flags = nullptr; return VLOAM_ERR_HIP; }
    for (int k = 0; k < 2 * kMaxBatch; k++) m->host_flags[k] = 0;
  }
  for (int k = 0; k < 2; k++) {
    if (m->pub.pub_number > 0 && !m->pub.ev_map[k] && hipEventCreateWithFlags(&m->pub.ev_map[k], hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) return VLOAM_ERR_HIP;
    if (m->pub.cloud_on && !m->pub.ev_cloud[k] && hipEventCreateWithFlags(&m->pub.ev_cloud[k], hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) return VLOAM_ERR_HIP;
  }
  MapState init;
  memset(&init, 0, sizeof(init));
  init.parameters[3] = 1.0; init.q_wmap_wodom[3] = 1.0; init.q_wodom_curr[3] = 1.0;  // LM:74-91
  init.cenW = 10; init.cenH = 10; init.cenD = 5;                                      // laser_mapping.h:76-78
  if (hipMemcpyAsync(m->state, &init, sizeof(init), hipMemcpyHostToDevice, st) != hipSuccess) return VLOAM_ERR_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

void map_destroy(MapContext* m) {
  map_localize_free(m);
  map_carve_free(m);
  map_archive_free(m);
  if (m->grow) map_grow_destroy(m);
  if (m->host_flags) { (void)hipHostFree(m->host_flags); m->host_flags = nullptr; }
  for (int k = 0; k < 2; k++)
    for (hipEvent_t* e : {&m->pub.ev_map[k], &m->pub.ev_cloud[k]}) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
}

// gather the live records, clear the table, reinsert (see k_map_rebuild_*); between two sweeps on the mapping stream; one session
static vloam_status map_rebuild_enqueue(MapContext* m0, hipStream_t st, int session, int kind) {
  if (m0->grow) return map_grow_rehash(m0, st, kind);   // a fresh table of the same size (rebuild_tmp would not fit a grown one)
  MapContext ms_ = m0->for_session(session);
  MapContext* m = &ms_;
  VoxelTable& T = m->tab[kind];
  const size_t slots = (size_t)T.mask + 1, bslots = (size_t)T.bslots_mask + 1;
  const int cap = kind ? m->surf_cap : kStackCapCorner;
  if (hipMemsetAsync(m->rebuild_n, 0, sizeof(int), st) != hipSuccess) return VLOAM_ERR_HIP;
  VL_RAW_LAUNCH(k_map_rebuild_gather, dim3(1024), dim3(256), 0, st, T, m->rebuild_tmp, m->rebuild_cap, m->rebuild_n, m->frame, kind);
  if (hipMemsetAsync(T.rec, 0, slots * sizeof(VoxelRec), st) != hipSuccess) return VLOAM_ERR_HIP;
  if (hipMemsetAsync(T.blk, 0, bslots * sizeof(ulonglong2), st) != hipSuccess) return VLOAM_ERR_HIP;
  VL_RAW_LAUNCH(k_map_rebuild_insert, dim3(1024), dim3(256), 0, st, T, m->rebuild_tmp, m->rebuild_cap, m->rebuild_n, m->frame, kind,
                     m->deferred[kind], cap, m->host_flags);
  m0->rebuilds++;
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

vloam_status map_reclaim_enqueue(MapContext* m, hipStream_t st, int kind) { return map_rebuild_enqueue(m, st, 0, kind); }

vloam_status map_force_rebuild(MapContext* m, hipStream_t st) {
  for (int b = 0; b < m->se.B; b++)
    for (int k = 0; k < 2; k++) { vloam_status s = map_rebuild_enqueue(m, st, b, k); if (s != VLOAM_OK) return s; }
  return VLOAM_OK;
}

static const bool g_ts_log = getenv("VLOAM_TS_LOG") != nullptr;   // debug: device-side time stamps of the mapping stage (tools/map_stream_gaps.py)
vloam_status map_enqueue(MapContext* m, const vloam_config& cfg, hipStream_t st, const SRBuffers& cur, LOState* lo, double* traj_row14,
                         bool skip_frame, int set, ProfHook* ph, hipEvent_t done) {
  (void)cur;
  MapState* ms = m->state;
  MapFrame* fr = m->frame;
  const unsigned Z = (unsigned)m->se.B;
  const size_t ss = m->se.ss;
  m->stack[0] = m->stack_sets[set][0]; m->stack[1] = m->stack_sets[set][1];
  if (m->grow && !skip_frame && map_grow_before_sweep(m, st) != VLOAM_OK) return VLOAM_ERR_HIP;   // (no kernel of this sweep's mapping is enqueued yet)
  if (!skip_frame) {
    // the flag is written by k_map_finalize of an EARLIER sweep (plain read of host-mapped memory, no synchronisation): a rebuild
    // a few sweeps late is as good; the cool-down covers the sweeps already in flight that still report the old state
    for (int b = 0; b < m->se.B; b++)
      for (int k = 0; k < 2; k++) {
        if (m->rebuild_cooldown[b][k] > 0) { m->rebuild_cooldown[b][k]--; continue; }
        if (__atomic_load_n(&m->host_flags[2 * b + k], __ATOMIC_RELAXED)) {
          if (map_rebuild_enqueue(m, st, b, k) != VLOAM_OK) return VLOAM_ERR_HIP;
          m->rebuild_cooldown[b][k] = 8;
        }
      }
  }
  // `done` (mapping of this sweep finished) rides on the sweep's last dispatch: a marker packet behind it costs ~5 us of idle stream
  // A handle of the large stack tier (surf capacity S > kStackCapSurf) launches the *_tier forms — the same bodies with S at run time — under
  // the same kernel ids, on grids sized by S; a default handle launches exactly what it always did.
  const bool tier = m->tier();
  const int S = m->surf_cap;
#define VL_PREPARE(KERN, ...)                                                                                                                          \
  VLOAM_LAUNCH_EV(ph, kKMapPrepare, st, skip_frame ? done : nullptr, KERN, dim3(1, 1, Z), dim3(256), 0, st, ms, fr, lo, m->cube_cnt, skip_frame ? 1 : 0, \
                  traj_row14, m->stack_info[set], m->deferred[0], m->deferred[1], m->newraw[0], m->newraw[1], g_ts_log ? m->ts_log : (long long*)nullptr, __VA_ARGS__)
  if (tier) VL_PREPARE(k_map_prepare_tier, ss, S);
  else VL_PREPARE(k_map_prepare, ss);
#undef VL_PREPARE
  if (skip_frame) return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
  m->pub.mapped++;
  if (m->archive) map_archive_enqueue(m, st);   // the points of cubes this sweep's roll evicts, before k_map_finalize purges them (map_archive.hip)
  for (int outer = 0; outer < 2; outer++) {  // LM:458
    // lanes per query of the 5-NN search: a batch fills the chip with 16-lane groups (four queries per wavefront); a single sequence
    // (9 000 queries on 5 120 wave slots) is quickest with two per wavefront.  VLOAM_MAP_ASSOC_LANES = 16 / 32 / 64 overrides (A/B runs;
    // the round-2 form — one wavefront per query, rank counting in LDS — measured 27.8 / 184 us at B = 1 / 8 against 16 / 105 here).
    static const int g_env = getenv("VLOAM_MAP_ASSOC_LANES") ? atoi(getenv("VLOAM_MAP_ASSOC_LANES")) : -1;
    const int G = g_env >= 0 ? g_env : (m->se.B > 1 ? 16 : 32);
    auto grid_for = [S](int g) { const int qw = 256 / g; return dim3(8 * ((kStackCapCorner / qw + 7) / 8 + (S / qw + 7) / 8), 1, 1); };   // (k_map_assoc itself bakes in the corner capacity only: the grid is what grows with the tier)
#define VL_MAP_ASSOC(KERN, GRID)                                                                                                      \
    VLOAM_LAUNCH(ph, kKMapAssoc, st, KERN, dim3((GRID).x, 1, Z), dim3(256), 0, st, m->stack[0], m->stack[1], m->tab[0], m->tab[1], \
                 m->inv_leaf[0], m->inv_leaf[1], ms, fr, m->nbr, outer, m->cbox, m->ccand, cfg.debug ? m->assoc_cyc : (long long*)nullptr, ss)
    static const int kb_env = getenv("VLOAM_MAP_ASSOC_KB") ? atoi(getenv("VLOAM_MAP_ASSOC_KB")) : 2;   // blocks per lane and trip of the 16-lane groups
    if (G == 16 && kb_env == 1) VL_MAP_ASSOC((k_map_assoc<16, 1>), grid_for(16));
    else if (G == 16) VL_MAP_ASSOC((k_map_assoc<16, 2>), grid_for(16));
    else if (G == 64) VL_MAP_ASSOC((k_map_assoc<64, 1>), grid_for(64));
    else VL_MAP_ASSOC((k_map_assoc<32, 1>), grid_for(32));
#undef VL_MAP_ASSOC
#define VL_FIT(KERN, GRID_X)                                                                                                               \
    VLOAM_LAUNCH(ph, kKMapFit, st, KERN, dim3((GRID_X), 1, Z), dim3(256), 0, st, m->stack[0], m->stack[1], m->tab[0], m->tab[1], ms, fr, m->nbr, \
                 m->F[outer], outer, ss)
    if (tier) VL_FIT(k_map_fit_tier, m->factor_cap() / 256);
    else VL_FIT(k_map_fit, kMapFactorCap / 256);
#undef VL_FIT
    lm_launch(st, m->se, m->F[outer], kStackCapCorner, ms->parameters, m->rec + outer, 4, 0.1, true, &ms->do_optimize, ph);
  }
#define VL_INSERT(KERN, ...)                                                                                                                  \
  VLOAM_LAUNCH(ph, kKMapInsert, st, KERN, dim3(64, 2, Z), dim3(256), 0, st, m->stack[0], m->stack[1], m->stack_map[0], m->stack_map[1], m->tab[0], \
               m->tab[1], m->inv_leaf[0], m->inv_leaf[1], ms, fr, m->touched[0], m->touched[1], m->deferred[0], m->deferred[1], traj_row14, __VA_ARGS__)
#define VL_FINALIZE(KERN, GRID_X, ...)                                                                                                           \
  VLOAM_LAUNCH_EV(ph, kKMapFinalize, st, done, KERN, dim3((GRID_X), 2, Z), dim3(256), 0, st, m->stack_map[0], m->stack_map[1], m->tab[0], m->tab[1], \
                  ms, fr, m->touched[0], m->touched[1], m->deferred[0], m->deferred[1], m->newraw[0], m->newraw[1], m->cube_cnt, m->host_flags,      \
                  g_ts_log ? m->ts_log : (long long*)nullptr, __VA_ARGS__)
  if (tier) { VL_INSERT(k_map_insert_tier, ss, S); VL_FINALIZE(k_map_finalize_tier, S / 256, ss, S); }
  else { VL_INSERT(k_map_insert, ss); VL_FINALIZE(k_map_finalize, kStackCapSurf / 256, ss); }
#undef VL_INSERT
#undef VL_FINALIZE
  if (m->grow) map_grow_progress_enqueue(m, st);
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

// A localisation (vloam_map_localize): map_enqueue's chain for a single sequence of the default stack tier up to the second solve, on the
// scratch of m->loc — k_map_loc_prepare for k_map_prepare, no insert, no finalize, k_map_loc_finish packs the record (map_localize.hip).
// The tables are m->tab[] as they are NOW, behind whatever growth step the last map_enqueue put on the stream.  No profiling hook: the
// per-kernel timer counts sweeps' launches.
vloam_status map_localize_enqueue(MapContext* m, hipStream_t st, const float4* corner, int n_corner, const float4* surf, int n_surf, int set,
                                  const double* row7, const double pose7[7], int pose_frame, vloam_localize_result* d_result) {
  MapLocalize* L = m->loc;
  const float4* stack[2] = {m->stack_sets[set][0], m->stack_sets[set][1]};
  const StackInfo* si = m->stack_info[set];
  if (corner || surf) {
    // counts and VoxelGrid boxes of the caller's clouds, then the VoxelGrid itself (the two launches of map_stack_enqueue)
    SRBuffers b{};
    b.S = L->S; b.less_sharp = const_cast<float4*>(corner); b.less_flat = const_cast<float4*>(surf);
    if (hipMemsetAsync(L->si, 0, sizeof(StackInfo), st) != hipSuccess) return VLOAM_ERR_HIP;
    sr_adopt_launch(st, b, -1, -1, n_corner, -1, n_surf);
    map_stack_enqueue_loc(m, st, corner, surf);
    stack[0] = L->stack[0]; stack[1] = L->stack[1];
    si = L->si;
  }
  map_loc_prepare_launch(st, m, si, row7, pose7, pose_frame);
  MapState* ms = L->state;
  MapFrame* fr = L->frame;
  Sess se = m->se;
  se.B = 1; se.ss = 0;
  for (int outer = 0; outer < 2; outer++) {
    const int qw = 256 / 32;
    VL_RAW_LAUNCH((k_map_assoc<32, 1>), dim3(8 * ((kStackCapCorner / qw + 7) / 8 + (kStackCapSurf / qw + 7) / 8), 1, 1), dim3(256), 0, st, stack[0], stack[1],
                  m->tab[0], m->tab[1], m->inv_leaf[0], m->inv_leaf[1], ms, fr, L->nbr, outer, L->cbox, L->ccand, (long long*)nullptr, (size_t)0);
    VL_RAW_LAUNCH(k_map_fit, dim3(kMapFactorCap / 256, 1, 1), dim3(256), 0, st, stack[0], stack[1], m->tab[0], m->tab[1], ms, fr, L->nbr, L->F[outer], outer,
                  (size_t)0);
    lm_launch(st, se, L->F[outer], kStackCapCorner, ms->parameters, L->rec + outer, 4, 0.1, true, &ms->do_optimize, nullptr);
  }
  map_loc_finish_launch(st, m, d_result);
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

}  // namespace vloam
