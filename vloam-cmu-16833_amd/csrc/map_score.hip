// Pose scoring on gfx950: M candidate poses x N feature points x one nearest-neighbour lookup in the map (vloam_map_score_poses /
// vloam_map_score_poses_device; the first step of vloam_map_relocalize).  A code object of its own (map_table.h and map_device.h are all it
// shares with the sweep's kernels): a handle that never scores launches nothing of this, and no kernel of a sweep changes.
//
// Per pose m, kind and used point i (points 0, s, 2s, ... of the kind's cloud): p = associate_to_map(point_i, q_m, t_m), the searched set is
// k_map_export's for that kind (map_walk.h), d2 = (dx*dx + dy*dy) + dz*dz in f32 with every product and sum rounded on its own, dmin the
// smallest d2; a hit when dmin <= r*r.  A record counts the hits and sums (u64)(dmin * 2^24) over them: integers, accumulated in registers,
// over the wave by shuffles and into the record by integer atomics, so a record is a function of the inputs alone whatever the launch geometry.
//
// Layout: the work is cut into (pose tile of kScPoses) x (point tile of kScPoints of one kind); a workgroup takes tiles grid-stride, stages the
// tile's points in LDS once, and each of its four waves takes every fourth pose of the tile into registers.  A group of kScG = 8 lanes covers
// one point's boxes (at radius 1 m and the default leaves a box is 27 blocks: three to four rounds of eight busy lanes, where 32 lanes would
// idle), so a wave scores eight points of one pose at a time and issues one 64-bit and one 32-bit atomic per pose and tile.
// The walk through the occupancy-block index — the box as per-axis pieces, the blocks, the voxel records, and why nothing the box can hold is
// left out — is map_walk.h's, shared with map_query.hip; every block of the box is visited (no early-out).
#include <hip/hip_runtime.h>
#include <math.h>
#include "map_walk.h"

namespace vloam {

namespace {

constexpr int kScG = 8;                    // lanes per (pose, point) pair
constexpr int kScGroups = 256 / kScG;      // 32 groups per workgroup, 8 per wave
constexpr int kScPoints = 64;              // points per tile (one kind)
constexpr int kScPoses = 16;               // poses per tile: four per wave
constexpr int kScMaxGrid = 4096;

}  // namespace

// every record: zero hits and sums, the points scored per kind
__global__ __launch_bounds__(256) void k_map_score_init(vloam_pose_score* __restrict__ out, int M, int nu0, int nu1) {
  for (int m = (int)(blockIdx.x * 256 + threadIdx.x); m < M; m += (int)gridDim.x * 256) {
    vloam_pose_score r;
    r.n_hit[0] = 0; r.n_hit[1] = 0; r.n_used[0] = nu0; r.n_used[1] = nu1; r.sum_d2_q24[0] = 0ull; r.sum_d2_q24[1] = 0ull;
    out[m] = r;
  }
}

// cloud0 / cloud1: the corner / surf cloud in the sensor frame; nu: used points per kind; poses: [M][7] (q xyzw, t).  Any M and N on a bounded grid.
__global__ __launch_bounds__(256) void k_map_score(VoxelTable T0, VoxelTable T1, float inv0, float inv1, const MapState* __restrict__ ms, MapFrame* fr,
                                                   const float4* __restrict__ cloud0, const float4* __restrict__ cloud1, int nu0, int nu1,
                                                   int stride0, int stride1, float radius0, float radius1, float r2_0, float r2_1,
                                                   const double* __restrict__ poses, int M, vloam_pose_score* __restrict__ out) {
  __shared__ float4 s_pt[kScPoints];
  __shared__ int s_piece[kScGroups][3][kWalkPieces];
  __shared__ int s_np[kScGroups][4];   // pieces per axis | more pieces than the table holds
  const int lane = threadIdx.x & 63, gl = lane & (kScG - 1), gi = threadIdx.x / kScG, wave = threadIdx.x >> 6, gw = lane / kScG;
  const int cen0 = ms->cenW, cen1 = ms->cenH, cen2 = ms->cenD;
  const int tiles0 = (nu0 + kScPoints - 1) / kScPoints, tiles1 = (nu1 + kScPoints - 1) / kScPoints, ptiles = tiles0 + tiles1;
  const int mtiles = (M + kScPoses - 1) / kScPoses;
  const long long total = (long long)ptiles * (long long)mtiles;
  bool chain_too_long = false, piece_overflow = false;
  for (long long tile = blockIdx.x; tile < total; tile += gridDim.x) {   // workgroup-uniform
    const int mt = (int)(tile / ptiles), pt = (int)(tile - (long long)mt * ptiles);
    const int kind = pt >= tiles0 ? 1 : 0;
    const int first = (kind ? pt - tiles0 : pt) * kScPoints;
    const int cnt = min(kScPoints, (kind ? nu1 : nu0) - first);   // >= 1
    const VoxelTable T = kind ? T1 : T0;
    const float inv = kind ? inv1 : inv0, radius = kind ? radius1 : radius0, r2 = kind ? r2_1 : r2_0;
    __syncthreads();   // the previous tile's readers are done
    if ((int)threadIdx.x < cnt) s_pt[threadIdx.x] = (kind ? cloud1 : cloud0)[(size_t)(first + (int)threadIdx.x) * (size_t)(kind ? stride1 : stride0)];
    __syncthreads();
    for (int pm = wave; pm < kScPoses; pm += 4) {   // wave-uniform
      const int m = mt * kScPoses + pm;
      if (m >= M) break;
      double q[4], t[3];
#pragma unroll
      for (int c = 0; c < 4; c++) q[c] = poses[(size_t)m * 7 + c];
#pragma unroll
      for (int c = 0; c < 3; c++) t[c] = poses[(size_t)m * 7 + 4 + c];
      int hits = 0;
      u64 sum = 0ull;
      for (int i0 = 0; i0 < cnt; i0 += 64 / kScG) {   // wave-uniform
        const int i = i0 + gw;
        const bool live = i < cnt;
        const float4 qp = associate_to_map(live ? s_pt[i] : make_float4(0.f, 0.f, 0.f, 0.f), q, t);
        // a non-finite point, or one far outside the +-25.6 km the voxel key spans (and outside what an int voxel index holds), is no hit
        const bool search = live && fabsf(qp.x) <= 1.0e6f && fabsf(qp.y) <= 1.0e6f && fabsf(qp.z) <= 1.0e6f;
        // ---- the box, per axis, as pieces (lane a of the group lists axis a)
        if (gl < 4) s_np[gi][gl] = 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (search && gl < 3) {
          const float qa = gl == 0 ? qp.x : (gl == 1 ? qp.y : qp.z);
          const int cen = gl == 0 ? cen0 : (gl == 1 ? cen1 : cen2), wdim = gl == 0 ? kCubeW : (gl == 1 ? kCubeH : kCubeD);
          const int np = walk_axis_pieces(qa, radius, inv, cen, wdim, gl == 2 ? kCubeOffZ : kCubeOffXY, s_piece[gi][gl]);
          s_np[gi][gl] = np;
          if (np < 0) s_np[gi][3] = 1;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int np0 = s_np[gi][0], np1 = s_np[gi][1], np2 = s_np[gi][2];
        const bool ovf = s_np[gi][3] != 0;
        piece_overflow = piece_overflow || ovf;
        const int nblocks = (search && !ovf) ? np0 * np1 * np2 : 0;
        // ---- blocks over the lanes of the group, voxels of a block one after the other
        float dmin = INFINITY;
        for (int bb = gl; bb < nblocks; bb += kScG) {
          const int n01 = np0 * np1;
          const int ez = bb / n01, rem = bb - ez * n01, ey = rem / np0, ex = rem - ey * np0;
          walk_block(T, s_piece[gi][0][ex], s_piece[gi][1][ey], s_piece[gi][2][ez], &chain_too_long, [&](const RecVal& v, unsigned) {
            const float4 c = rec_point(v);
            const float dx = qp.x - c.x, dy = qp.y - c.y, dz = qp.z - c.z;
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            if (d2 < dmin) dmin = d2;
          });
        }
        // ---- the group's minimum; its first lane counts the point
#pragma unroll
        for (int sh = kScG / 2; sh >= 1; sh >>= 1) {
          const float od = __shfl_xor(dmin, sh);
          dmin = od < dmin ? od : dmin;
        }
        if (gl == 0 && dmin <= r2) {
          hits++;
          sum += (u64)__fmul_rn(dmin, 16777216.0f);
        }
      }
      // ---- the wave's hits and quantised sum: integer adds over shuffles, then one 64-bit and one 32-bit atomic
#pragma unroll
      for (int sh = 32; sh >= kScG; sh >>= 1) {
        hits += __shfl_xor(hits, sh);
        sum += (u64)__shfl_xor((unsigned long long)sum, sh);
      }
      if (lane == 0 && hits != 0) {
        atomicAdd(&out[m].n_hit[kind], hits);
        atomicAdd(&out[m].sum_d2_q24[kind], sum);
      }
    }
  }
  // piece_overflow shares the map-full word with a probe chain at its bound, as in map_query.hip.  It cannot happen for a radius the entry points
  // accept: 16 leaves are at most 36 voxel indices per axis, 10 blocks, plus 2 per cube face crossed — about 12 of the kWalkPieces slots.
  if (__ballot(chain_too_long || piece_overflow) != 0ull && lane == 0) atomicOr(&fr->error, kErrMapFull);
}

// Enqueue only: records zeroed (n_used set) and scored on `st`, against the tables as they are on `st` at this point.  Single-sequence handles.
vloam_status map_score_enqueue(MapContext* m, hipStream_t st, const void* d_corner, int n_corner, const void* d_surf, int n_surf, const int stride[2],
                               const float radius[2], const double* d_q4t3, int M, void* d_out) {
  if (M <= 0) return VLOAM_OK;
  const int nu0 = n_corner > 0 ? (n_corner + stride[0] - 1) / stride[0] : 0, nu1 = n_surf > 0 ? (n_surf + stride[1] - 1) / stride[1] : 0;
  VL_RAW_LAUNCH(k_map_score_init, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (vloam_pose_score*)d_out, M, nu0, nu1);
  const long long total = (long long)((nu0 + kScPoints - 1) / kScPoints + (nu1 + kScPoints - 1) / kScPoints) * (long long)((M + kScPoses - 1) / kScPoses);
  if (total > 0) {
    const dim3 grid((unsigned)(total < kScMaxGrid ? total : kScMaxGrid));
    VL_RAW_LAUNCH(k_map_score, grid, dim3(256), 0, st, m->tab[0], m->tab[1], m->inv_leaf[0], m->inv_leaf[1], m->state, m->frame, (const float4*)d_corner,
                  (const float4*)d_surf, nu0, nu1, stride[0], stride[1], radius[0], radius[1], radius[0] * radius[0], radius[1] * radius[1], d_q4t3, M,
                  (vloam_pose_score*)d_out);
  }
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

}  // namespace vloam
