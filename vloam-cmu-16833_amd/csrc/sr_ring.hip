// k_sr_ring: the LDS-resident ring of the scan registration (SR:288-439; the whole stage: sr_kernels.hip), in its two capacity tiers
// (sr_ring.h).  One workgroup per ring: curvature, sort-free picks (wavefront arg-max rounds, six sectors at once + boundary fixed point),
// lessFlat + VoxelGrid(0.2) over voxel runs.  The rules it shares with the long tier (sr_ring_long.hip): sr_ring_dev.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <type_traits>
#include "sr_ring.h"
#include "bitonic.h"

namespace vloam {

constexpr int kRingWatch = 2144;               // the small tier's warning to the big tier: an HDL-64E revolution at 10 Hz has <= 2 083 firings per laser
constexpr int kLongWatch = kMaxRingLen - 32;   // the big tier's warning to the long tier (the same margin)

template <int CAP, int SECT, bool BIG_TIER>
__global__ __launch_bounds__(kRingThreads) void k_sr_ring(const float4* __restrict__ cloud, FrameScalars* S, int* __restrict__ sharp_idx,
                                                          int* __restrict__ less_sharp_idx, int* __restrict__ flat_idx,
                                                          float4* __restrict__ ring_ds, float* __restrict__ dbg_curv,
                                                          int* __restrict__ dbg_sort, int* __restrict__ dbg_picked,
                                                          int* __restrict__ dbg_label, long long* __restrict__ dbg_cyc /* [rings][8] */,
                                                          int* ring_watch /* host-mapped [2][kMaxBatch] */, int tier_follows, size_t ss) {
  VL_SESSION(ss); RB(cloud); RB(S); RB(sharp_idx); RB(less_sharp_idx); RB(flat_idx); RB(ring_ds); RB(dbg_curv); RB(dbg_sort); RB(dbg_picked);
  RB(dbg_label); RB(dbg_cyc);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using L = SrRingLds<CAP, SECT>;
  float *px = (float*)(smem + L::px), *py = (float*)(smem + L::py), *pz = (float*)(smem + L::pz), *pi = (float*)(smem + L::pi);
  u64* keys = (u64*)(smem + L::keys);
  int *iscratch = (int*)(smem + L::iscratch), *scan_tmp = (int*)(smem + L::scan_tmp);
  unsigned char *picked = smem + L::picked, *gap = smem + L::gap, *reachb = smem + L::reach;
  signed char* label = (signed char*)(smem + L::label);
  int *s_sp = (int*)(smem + L::sp), *s_ep = (int*)(smem + L::ep), *s_leak_lo = (int*)(smem + L::leak_lo), *s_leak_hi = (int*)(smem + L::leak_hi);
  int *s_zone = (int*)(smem + L::zone), *s_any = (int*)(smem + L::any);
  const auto get = [=](int l) { return make_float4(px[l], py[l], pz[l], pi[l]); };   // point l of the ring

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // One workgroup per ring (gridDim.x == kMaxRings) — or, as the catch-all behind the small tier on sweeps for which the host has
  // not launched the full big tier, ONE workgroup per session that walks the rings and works on the (normally zero) oversized ones.
  auto one_ring = [&](const int r) {
  long long tstamp[8];
  int nstamp = 0;
#define SR_STAMP() do { if (dbg_cyc) tstamp[nstamp] = clock64(); nstamp++; } while (0)
  SR_STAMP();
  const int len = S->ring_count[r], off = S->ring_off[r];
  const int start = off + 5, end = off + len - 6;  // SR:278-280
  if (BIG_TIER && len <= kRingCapSmall) return;    // the small tier has done this ring
  if (tid < kSectors * 3) (&S->sect_cnt[r][0][0])[tid] = 0;
  if (tid == 0) S->ring_ds_cnt[r] = 0;
  // The big tier asks for 146 KB of LDS just to start, which on a busy chip (batches) costs tens of microseconds even when it has
  // nothing to do: the host only launches its full grid while rings near the small tier's capacity have been seen (ring_watch, a
  // host-mapped word it polls without synchronising) or during the first sweeps; otherwise a single catch-all workgroup per session
  // follows the small tier, so that a ring which outgrows the small tier without that warning is still processed (slowly: the rings
  // one after the other, until the host has seen the watch word).
  // The same between the big tier and the long tier (k_sr_ring_long, long-tier handles only): the big tier raises the second watch word
  // (ring_watch[kMaxBatch + session]) for rings near kMaxRingLen, which the host only reads on handles that have a long tier.
  if (!BIG_TIER && tid == 0 && len > kRingWatch && ring_watch) __hip_atomic_store(&ring_watch[blockIdx.z], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (BIG_TIER && tid == 0 && len > kLongWatch && ring_watch) __hip_atomic_store(&ring_watch[kMaxBatch + blockIdx.z], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // tier_follows: the next tier is launched behind this one (small tier: the big tier; big tier: the long tier) and takes what does not fit
  if (len > CAP) { if (!tier_follows && tid == 0) atomicOr(&S->error, kErrRingTooLong); return; }
  if (end - start < 6) return;  // SR:314

  for (int l = tid; l < len; l += kRingThreads) {
    float4 p = cloud[off + l];
    px[l] = p.x; py[l] = p.y; pz[l] = p.z; pi[l] = p.w;
    picked[l] = 0; label[l] = 0;  // SR:305-306
  }
  if (tid < kSectors) {
    s_sp[tid] = sr_sector_lo(start, end, tid);
    s_ep[tid] = sr_sector_hi(start, end, tid);
  }
  __syncthreads();
  SR_STAMP();

  // ---- neighbour-suppression reach of every point, computed once in parallel (SR:353-376 walks outwards while consecutive
  // points are close): gap bit l = sr_gap(p[l], p[l + 1]); reach[l] = (how many of l-1..l-5) |
  // (how many of l+1..l+5) << 4 a pick at l would mark.  The gap bits of 64 consecutive points are one ballot word; a point then
  // reads its five bits forward and five bits backward out of three words (count of trailing / leading zeros) instead of walking up to
  // ten bytes, each a dependent LDS round trip.
  u64* gapw = (u64*)gap;   // [CAP / 64 + 1] ballot words (the byte array's place)
  for (int base = wave * 64; base < len; base += kRingThreads) {   // wavefront-uniform
    const int l = base + lane;
    const bool g = l + 1 < len ? sr_gap(get(l), get(l + 1)) : true;
    const u64 m = __ballot(g);
    if (lane == 0) gapw[base >> 6] = m;
  }
  __syncthreads();
  for (int l = 5 + tid; l < len - 5; l += kRingThreads) {  // picks are >= 5 away from both ring ends
    const int c = l >> 6, b = l & 63;
    const u64 w0 = gapw[c], wn = gapw[c + 1], wp = c > 0 ? gapw[c - 1] : 0ull;
    // forward: bits l .. l+4 (SR:353-364 stops at the first gap)
    const unsigned fw = (unsigned)(((w0 >> b) | ((wn << 1) << (63 - b))) & 31ull);
    const int f = min(5, (int)__builtin_ctz(fw | 32u));
    // backward: bits l-1 .. l-5, bit l-1 on top (SR:365-376)
    const unsigned bw = b >= 5 ? (unsigned)((w0 >> (b - 5)) & 31ull) : (unsigned)(((wp >> (59 + b)) | (w0 << (5 - b))) & 31ull);
    const int k = min(5, (int)__builtin_clz((bw << 27) | (1u << 26)));
    reachb[l] = (unsigned char)(k | (f << 4));
  }

  // ---- debug only: the reference's std::sort of every sector (SR:323, canonical tie order: index ascending), as a
  // wavefront-local bitonic network in LDS.  The production path below never sorts.
  if (dbg_sort && wave < kSectors) {
    const int sp = s_sp[wave] - off, ep = s_ep[wave] - off;  // local indices
    const int seclen = ep - sp + 1;
    int P = 2;
    while (P < seclen) P <<= 1;
    u64* K = keys + wave * SECT;
    for (int t = lane; t < P; t += 64) {
      u64 key = ~0ull;
      if (t < seclen) key = ((u64)__float_as_uint(sr_curvature(get, sp + t)) << 32) | (unsigned)(sp + t);  // c >= 0: bits order like the value
      K[t] = key;
    }
    lds_fence_wave();
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        bitonic_stage(K, P, j, k, lane, 64);
        lds_fence_wave();
      }
    for (int t = lane; t < seclen; t += 64) dbg_sort[off + sp + t] = off + (int)(K[t] & 0xffffffffu);
  }
  __syncthreads();
  SR_STAMP();

  // ---- greedy picks (SR:325-422).  The reference sorts each sector by curvature and walks the sorted list from the top (2
  // sharp + 18 less-sharp picks) and from the bottom (4 flat picks), skipping points suppressed by earlier picks.  Walking a
  // sorted list and taking the first eligible entry is the same as taking the arg-max (arg-min) over the eligible entries,
  // and at most 24 entries are ever taken — so nothing is sorted: every lane keeps the curvatures of its sector points in
  // registers (point t of the sector lives in lane t % 64, slot t / 64) with one eligibility bit each, and a pick is one
  // wavefront arg-max (two DPP reductions: curvature bits, then index among the ties — descending (c, index) order for the
  // sharp walk, ascending for the flat walk, exactly the sorted list's order).
  //
  // The sectors of a ring are walked in order by the reference and a pick's neighbour suppression can spill over the sector
  // boundary (SR:353-376), so sector s + 1 formally depends on sector s.  The spill reaches at most 5 points and only
  // matters if one of them would otherwise be selected, so all six sectors run at once (one wavefront each) without incoming
  // marks; afterwards the boundaries are checked in order and a sector is redone — with the marks of its predecessor applied
  // first — only when a spilled-on point had been selected.  Marks are clipped to the own sector while picking (a later
  // sector must not disturb an earlier one); the full extents are applied at the end so that `picked` ends up exactly like
  // cloudNeighborPicked.
  // A redone sector does not start over: its picks are taken in priority order, so every pick made BEFORE the first one the new spill
  // invalidates stands — the picks of both walks are kept in LDS, the kept ones are replayed (marks only, all at once, one lane each)
  // and the walk resumes behind them.  On average half of the second pass; a spill that hits a flat pick keeps the whole sharp walk.
  unsigned* cbits = (unsigned*)keys;      // [CAP] curvature bits of the sector points (a redo reads them back instead of 33 LDS reads per point)
  constexpr int kPickSlots = kMaxLessSharpPerSect + kMaxFlatPerSect;
  int* s_plist = iscratch + 64;                         // [kSectors][kPickSlots] local index of the walks' picks, in pick order
  int* s_pcnt = s_plist + kSectors * kPickSlots;        // [kSectors][2] picks of the sharp / flat walk
  auto run_sector_q = [&](auto kq_tag, int s, int in_hi, bool redo, int keep_sharp, bool sharp_final, int keep_flat) {
    constexpr int kQ = decltype(kq_tag)::value;   // register slots per lane: sector length <= 64 kQ
    // (the same in every lane: in scalar registers, so that what derives from them — the lane masks of suppress() — is scalar too)
    const int sp_l = __builtin_amdgcn_readfirstlane(s_sp[s] - off), ep_l = __builtin_amdgcn_readfirstlane(s_ep[s] - off);
    const int seclen = ep_l - sp_l + 1;
    int* plist = s_plist + s * kPickSlots;
    if (redo) {  // forget the previous result, then apply the predecessor's spill
      for (int l = sp_l + lane; l <= ep_l; l += 64) { picked[l] = (l <= in_hi) ? 1 : 0; label[l] = 0; }
      lds_fence_wave();
    }
    // A pick is a chain of dependent instructions on a wavefront that is (almost) alone on its SIMD — ~8 cycles each —, so the walk is
    // written for few instructions per pick: the lane's candidates are kept PRE-MASKED (an ineligible slot holds the walk's neutral
    // value: the lane's best is a max3 / min3 tree), the winner's local index travels with its suppression reach in one word (no LDS
    // round trip for the reach), the lane that owns the winner is found by ballot (a second reduction only when two lanes tie), and the
    // picks stay in registers (lane k: pick k) until the walk is over — labels, index lists and the pick list are written once, in parallel.
    unsigned cb[kQ];                      // curvature bits of point sp_l + q * 64 + lane
    unsigned pay[kQ];                     // its local index << 8 | reach byte
    unsigned sharp_bits = 0, flat_bits = 0, elig = 0, inside = 0;
#pragma unroll
    for (int q = 0; q < kQ; q++) {
      cb[q] = 0; pay[q] = 0;
      if (q * 64 < seclen) {
        const int t = q * 64 + lane;
        if (t < seclen) {
          const int i = sp_l + t;
          inside |= 1u << q;
          if (redo) {
            cb[q] = cbits[i];
          } else {
            const float c0 = sr_curvature(get, i);
            if (dbg_curv) dbg_curv[off + i] = c0;
            cb[q] = __float_as_uint(c0);   // c >= 0: the bit pattern orders like the value
            cbits[i] = cb[q];
          }
          pay[q] = ((unsigned)i << 8) | (unsigned)reachb[i];
          if (sr_sharp_cand(cb[q])) sharp_bits |= 1u << q;   // SR:330
          if (sr_flat_cand(cb[q])) flat_bits |= 1u << q;     // SR:383
          if (i > in_hi) elig |= 1u << q;
        }
      }
    }
    int* o_sharp = sharp_idx + (r * kSectors + s) * kMaxSharpPerSect;
    int* o_less = less_sharp_idx + (r * kSectors + s) * kMaxLessSharpPerSect;
    int* o_flat = flat_idx + (r * kSectors + s) * kMaxFlatPerSect;
    int n_less = 0, n_flat = 0;
    unsigned my_sharp = 0, my_flat = 0;   // lane k: pick k of the sharp / flat walk (local index << 8 | reach)
    int leak_lo = INT_MAX, leak_hi = -1;
    unsigned v[kQ];                       // the running walk's pre-masked candidates
    // SR:353-376 around the winner, as far as the walk itself needs it: the (at most 11) covered points of the sector leave the
    // candidates.  The marks themselves (cloudNeighborPicked) are written after the walk, by one lane per pick.
    auto suppress = [&](unsigned pw, unsigned neutral) {
      const int lf = (int)(pw >> 8);
      const int lo_m = lf - (int)(pw & 15u), hi_m = lf + (int)((pw >> 4) & 15u);
      const int tlo = max(lo_m - sp_l, 0), thi = min(hi_m - sp_l, seclen - 1);
      const unsigned d = (unsigned)(lane - tlo), span = (unsigned)(thi - tlo);
#pragma unroll
      for (int q = 0; q < kQ; q++)
        if (d + (unsigned)(q * 64) <= span) v[q] = neutral;
    };
    // the marks (clipped to the sector) and extents of picks [from, to) of a walk: lane k marks around pick k
    auto apply_marks = [&](unsigned my, int from, int to) {
      int lo_m = INT_MAX, hi_m = -1;
      if (lane >= from && lane < to) {
        const int lf = (int)(my >> 8);
        lo_m = lf - (int)(my & 15u); hi_m = lf + (int)((my >> 4) & 15u);
        for (int l = max(lo_m, sp_l); l <= min(hi_m, ep_l); l++) picked[l] = 1;
      }
      leak_lo = min(leak_lo, (int)wave_min_u32((unsigned)lo_m));
      leak_hi = max(leak_hi, (int)wave_max_u32((unsigned)(hi_m + 1)) - 1);
    };
    // which of the lane's points no pick has marked (the walks themselves only keep v[] current)
    auto refresh_elig = [&]() {
      lds_fence_wave();
#pragma unroll
      for (int q = 0; q < kQ; q++)
        if (((inside >> q) & 1u) && picked[sp_l + q * 64 + lane]) elig &= ~(1u << q);
    };
    // kept picks [first, first + n) of the pick list come back into the registers (lane k: pick k); the first n_marking of them mark
    auto replay = [&](int first, int n, int n_marking, int sharp_walk) {
      unsigned my = 0;
      if (lane < n) { const int lf = plist[first + lane]; my = ((unsigned)lf << 8) | (unsigned)reachb[lf]; }
      if (sharp_walk) my_sharp = my; else my_flat = my;
      apply_marks(my, 0, n_marking);
    };
    // SR:327-378, descending curvature
    if (keep_sharp > 0) { replay(0, keep_sharp, keep_sharp, 1); n_less = keep_sharp; }
    if (!sharp_final) {
      if (redo) refresh_elig();
#pragma unroll
      for (int q = 0; q < kQ; q++) v[q] = ((elig & sharp_bits) >> q) & 1u ? cb[q] : 0u;   // candidates have c > 0.1, i.e. non-zero bits
      for (int picks = keep_sharp + 1; picks <= kMaxLessSharpPerSect; picks++) {
        unsigned lb = v[0];
#pragma unroll
        for (int q = 1; q < kQ; q++) lb = max(lb, v[q]);
        const unsigned mh = wave_max_u32(lb);
        if (mh == 0) break;
        unsigned pl = 0;
#pragma unroll
        for (int q = 0; q < kQ; q++) if (v[q] == mh) pl = pay[q];   // ascending: the higher index wins ties
        const u64 tie = __ballot(lb == mh);
        const unsigned pw = (tie & (tie - 1ull)) == 0ull ? (unsigned)__builtin_amdgcn_readlane((int)pl, __ffsll((long long)tie) - 1) : wave_max_u32(pl);
        if (lane == n_less) my_sharp = pw;
        n_less++;
        suppress(pw, 0u);
      }
      apply_marks(my_sharp, keep_sharp, n_less);
    }
    // SR:380-422, ascending curvature
    if (keep_flat > 0) { replay(kMaxLessSharpPerSect, keep_flat, min(keep_flat, kMaxFlatPerSect - 1), 0); n_flat = keep_flat; }
    refresh_elig();
#pragma unroll
    for (int q = 0; q < kQ; q++) v[q] = ((elig & flat_bits) >> q) & 1u ? cb[q] : 0xffffffffu;   // (c < 0.1: never all ones)
    for (int picks = keep_flat + 1;; picks++) {
      unsigned lb = v[0];
#pragma unroll
      for (int q = 1; q < kQ; q++) lb = min(lb, v[q]);
      const unsigned mh = wave_min_u32(lb);
      if (mh == 0xffffffffu) break;
      unsigned pl = 0xffffffffu;
#pragma unroll
      for (int q = kQ - 1; q >= 0; q--) if (v[q] == mh) pl = pay[q];   // descending: the lower index wins ties
      const u64 tie = __ballot(lb == mh);
      const unsigned pw = (tie & (tie - 1ull)) == 0ull ? (unsigned)__builtin_amdgcn_readlane((int)pl, __ffsll((long long)tie) - 1) : wave_min_u32(pl);
      if (lane == n_flat) my_flat = pw;
      n_flat++;
      if (picks >= kMaxFlatPerSect) break;  // the 4th flat point is emitted but not suppressed (SR:390-394)
      suppress(pw, 0xffffffffu);
    }
    apply_marks(my_flat, keep_flat, min(n_flat, kMaxFlatPerSect - 1));
    // labels, index lists, pick list: one lane per pick
    const int n_sharp = min(n_less, kMaxSharpPerSect);
    if (lane < n_less) {
      const int lf = (int)(my_sharp >> 8);
      label[lf] = lane < kMaxSharpPerSect ? 2 : 1;
      o_less[lane] = off + lf; plist[lane] = lf;
      if (lane < n_sharp) o_sharp[lane] = off + lf;
    }
    if (lane < n_flat) { const int lf = (int)(my_flat >> 8); label[lf] = -1; o_flat[lane] = off + lf; plist[kMaxLessSharpPerSect + lane] = lf; }
    lds_fence_wave();
    if (lane == 0) {
      S->sect_cnt[r][s][0] = n_sharp; S->sect_cnt[r][s][1] = n_less; S->sect_cnt[r][s][2] = n_flat;
      s_leak_lo[s] = leak_lo; s_leak_hi[s] = leak_hi;
      s_zone[s] = in_hi;
      s_pcnt[2 * s] = n_less; s_pcnt[2 * s + 1] = n_flat;
    }
  };
  auto run_sector = [&](int s, int in_hi, bool redo, int keep_sharp, bool sharp_final, int keep_flat) {
    if (s_ep[s] - s_sp[s] + 1 <= 6 * 64) run_sector_q(std::integral_constant<int, 6>{}, s, in_hi, redo, keep_sharp, sharp_final, keep_flat);   // HDL-64E: ~330 points per sector
    else run_sector_q(std::integral_constant<int, SECT / 64>{}, s, in_hi, redo, keep_sharp, sharp_final, keep_flat);
  };
  if (wave < kSectors) run_sector(wave, -1, false, 0, false, 0);
  __syncthreads();
  SR_STAMP();
  // fixed point over the boundaries: a sector is redone when the spill it was computed with differs from its predecessors'
  // current spill in a way that can matter.  Sector 0 never changes, so after round k sectors 0..k are final.
  for (int round = 0; round < kSectors - 1; round++) {
    if (tid == 0) *s_any = 0;
    __syncthreads();
    bool redo = false, sharp_final = false;
    int in_hi = -1, keep_sharp = 0, keep_flat = 0;
    if (wave >= 1 && wave < kSectors) {
      const int sp_l = s_sp[wave] - off, ep_l = s_ep[wave] - off;
      for (int q = 0; q < wave; q++) in_hi = max(in_hi, s_leak_hi[q]);  // a spill reaches 5 points: several sectors when they are tiny
      in_hi = min(in_hi, ep_l);
      if (in_hi < sp_l) in_hi = -1;
      const int used = s_zone[wave];
      if (in_hi > used) {        // the spill grew: matters only if a newly covered point (at most 5) had been selected
        const int nl = s_pcnt[2 * wave], nf = s_pcnt[2 * wave + 1];
        int lf = -1;
        if (lane < kMaxLessSharpPerSect) { if (lane < nl) lf = s_plist[wave * kPickSlots + lane]; }
        else if (lane < kPickSlots) { if (lane - kMaxLessSharpPerSect < nf) lf = s_plist[wave * kPickSlots + lane]; }
        const unsigned long long hit = __ballot(lf > used && lf <= in_hi);   // (picks lie inside the sector, i.e. at or above sp_l)
        redo = hit != 0ull;
        if (redo) {   // everything picked before the first invalidated pick stands
          const int k = __ffsll((long long)hit) - 1;
          if (k < kMaxLessSharpPerSect) { keep_sharp = k; }
          else { keep_sharp = nl; sharp_final = true; keep_flat = k - kMaxLessSharpPerSect; }
        }
        if (!redo && lane == 0) s_zone[wave] = in_hi;
      } else if (in_hi < used) {  // the spill shrank: points that were blocked are free again — from the start
        redo = true;
      }
      if (redo && lane == 0) *s_any = 1;
    }
    __syncthreads();  // every wavefront has read its predecessor's spill before anything is redone
    if (*s_any == 0) break;
    if (redo) run_sector(wave, in_hi, true, keep_sharp, sharp_final, keep_flat);
    __syncthreads();
  }
  if (wave == 0) {
    // full mark extents (beyond the own sector), as the reference leaves them behind
    for (int s = 0; s < kSectors; s++) {
      const int sp_l = s_sp[s] - off, ep_l = s_ep[s] - off;
      const int lo_m = s_leak_lo[s], hi_m = s_leak_hi[s];
      if (hi_m < 0) continue;
      if (lane < 8) {
        const int lb = lo_m + lane, lf = ep_l + 1 + lane;
        if (lb < sp_l) picked[lb] = 1;
        if (lf <= hi_m) picked[lf] = 1;
      }
    }
  }
  __syncthreads();
  SR_STAMP();
  sr_dump_marks(dbg_picked, dbg_label, off, len, picked, label);

  // ---- lessFlat (SR:424-430) + per-ring pcl::VoxelGrid leaf 0.2 (SR:433-437)
  const int c_lo = 5, c_hi = len - 7;  // local range covered by the six sectors: [start, end-1]
  const SrBox box = sr_lessflat_box(get, label, c_lo, c_hi, (float*)scan_tmp);
  const int ncand = box.ncand;
  if (ncand == 0) return;
  float4* out = ring_ds + (size_t)r * kMaxRingLen;
  if (SrGrid::too_fine(box)) { sr_ds_passthrough(get, label, len, c_lo, c_hi, iscratch, scan_tmp, out, S, r, ncand); return; }
  const SrGrid grid(box);
  // Consecutive ring points mostly fall into the same 0.2 m voxel, so the sort runs over RUNS (maximal stretches of
  // consecutive candidates sharing a voxel), not points: key = (voxel index, first point of the run).  Sorted runs of one
  // voxel are in input order and so are the points inside a run, hence summing run after run reproduces the
  // input-order f32 sums of pcl::VoxelGrid exactly, with a network several times smaller.
  // run key = voxel index : first point : last point (32 : 20 : 12 bits; a run is known by its first point, so the order is (voxel,
  // first point)).  The run's head writes the voxel and its own position, the point behind its last point ORs in where the run ended:
  // the centroid pass below then walks [first, last] without testing every point's voxel (a dependent LDS trip per point otherwise).
  //
  // Every wavefront takes a CONTIGUOUS stretch of the ring, 64 consecutive points per trip: a point's predecessor sits in the lane
  // below, the run heads of a trip are one ballot word and a head's run number is a population count — no voxel array, no flag array,
  // no workgroup scan (that was five passes over LDS behind five barriers; this is two passes behind two).
  u64* K2 = keys;                      // [<= CAP] run keys
  unsigned* K2w = (unsigned*)K2;       // [2 t] low word, [2 t + 1] high word
  constexpr int kTrips = (CAP + kRingThreads - 1) / kRingThreads;
  const int seg = ((len + kRingThreads - 1) / kRingThreads) * 64;   // points per wavefront (<= 64 kTrips)
  const int seg0 = wave * seg;
  auto voxel_of = [&](int l) -> int {  // -1: not a lessFlat candidate
    if (l < c_lo || l > c_hi || label[l] > 0) return -1;
    return grid.voxel_of(px[l], py[l], pz[l]);
  };
  int vidx[kTrips];
  u64 headm[kTrips], pcandm[kTrips];   // trip's run heads / lanes whose predecessor is a candidate
  int nheads = 0;
  {
    int carry = seg0 > 0 && seg0 - 1 < len ? voxel_of(seg0 - 1) : -2;   // the point in front of the stretch (-2: none)
    carry = __builtin_amdgcn_readfirstlane(carry);
#pragma unroll
    for (int it = 0; it < kTrips; it++) {
      vidx[it] = -1; headm[it] = 0ull; pcandm[it] = 0ull;
      if (it * 64 < seg) {
        const int l = seg0 + it * 64 + lane;
        const int v = l < len ? voxel_of(l) : -1;
        int pv = __shfl_up(v, 1);
        if (lane == 0) pv = carry;
        carry = __builtin_amdgcn_readlane(v, 63);
        vidx[it] = v;
        headm[it] = __ballot(v >= 0 && pv != v);
        pcandm[it] = __ballot(pv >= 0);
        nheads += __popcll(headm[it]);
        if (l < CAP) K2[l] = 0ull;   // (run numbers never exceed point numbers: every key that will be ORed together starts from zero)
      }
    }
  }
  int* s_heads = scan_tmp + 64;        // [8] (behind the bounding-box slots: a slow wavefront may still be reading those)
  if (lane == 0) s_heads[wave] = nheads;
  __syncthreads();
  int nrun = 0, running = 0;
  for (int w = 0; w < kRingThreads / 64; w++) { const int t = s_heads[w]; running += w < wave ? t : 0; nrun += t; }
  int P2 = 2;
  while (P2 < nrun) P2 <<= 1;
  for (int t = nrun + tid; t < P2 && t < CAP; t += kRingThreads) K2[t] = ~0ull;   // the sorting network's padding
#pragma unroll
  for (int it = 0; it < kTrips; it++) {
    if (it * 64 < seg) {
      const int l = seg0 + it * 64 + lane;
      const int v = vidx[it];
      const u64 hm = headm[it];
      const bool head = (hm >> lane) & 1ull;
      const int run = running + __popcll(hm & ((1ull << lane) - 1ull));   // heads in front of l
      if (head) { K2w[2 * run + 1] = (unsigned)v; atomicOr(&K2w[2 * run], (unsigned)l << 12); }
      if (((pcandm[it] >> lane) & 1ull) && (head || v < 0)) atomicOr(&K2w[2 * (run - 1)], (unsigned)(l - 1));   // l - 1 closed its run
      running += __popcll(hm);
    }
  }
  __syncthreads();
  SR_STAMP();
  // a stage with stride j <= 64 only moves data inside 128-element blocks that belong to one wavefront (64 consecutive
  // compare-exchanges), so only the wide strides need a workgroup barrier
  if (P2 > CAP) {
    // More runs than the largest power of two the key array holds (only the small tier's 2 176-point rings can get here, with a
    // voxel of its own for almost every point): rank by counting instead of padding the network to 4 096 keys.  Keys are unique.
    constexpr int NQ = (CAP + kRingThreads - 1) / kRingThreads;
    u64 mine[NQ];
    int rk[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int t = tid + q * kRingThreads;
      mine[q] = t < nrun ? K2[t] : ~0ull;
      int below = 0;
      if (t < nrun) for (int e = 0; e < nrun; e++) below += K2[e] < mine[q];
      rk[q] = below;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; q++) if (tid + q * kRingThreads < nrun) K2[rk[q]] = mine[q];
  } else if (P2 < 128) {
    for (int k = 2; k <= P2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        bitonic_stage(K2, P2, j, k, tid, kRingThreads);
        const int next_j = j > 1 ? j >> 1 : k;  // first stride of the next merge level
        if (j > 64 || next_j > 64) __syncthreads(); else lds_fence_wave();
      }
  } else if (P2 < 256 * (kRingThreads / 64)) {
    // up to 1 024 keys: 128-key blocks (two keys per lane) keep all eight wavefronts busy; strides <= 64 run in registers, the strides >= 128
    // go through LDS behind a workgroup barrier
    bitonic_reg_stages(K2, P2, 2, 128, tid, kRingThreads);
    __syncthreads();
    for (int k = 256; k <= P2; k <<= 1) {
      for (int j = k >> 1; j >= 128; j >>= 1) {
        bitonic_stage(K2, P2, j, k, tid, kRingThreads);
        __syncthreads();
      }
      bitonic_reg_stages(K2, P2, k, k, tid, kRingThreads);
      __syncthreads();
    }
  } else {
    // 2 048 keys and more: 256-key blocks (four keys per lane, one block per wavefront at 2 048); strides <= 128 run in registers, only the
    // strides >= 256 — 6 of the 66 stages at 2 048 run keys — go through LDS (41.5 k -> 37 k cycles; at 1 024 keys the wider blocks would
    // leave four wavefronts idle: 19 k -> 26 k)
    bitonic_reg_stages4(K2, P2, 2, 256, tid, kRingThreads);
    __syncthreads();
    for (int k = 512; k <= P2; k <<= 1) {
      for (int j = k >> 1; j >= 256; j >>= 1) {
        bitonic_stage(K2, P2, j, k, tid, kRingThreads);
        __syncthreads();
      }
      bitonic_reg_stages4(K2, P2, k, k, tid, kRingThreads);
      __syncthreads();
    }
  }
  __syncthreads();
  SR_STAMP();
  // voxel heads -> output rank, the same way (contiguous stretches of the sorted keys, ballot words, population counts), then the centroids
  int nvox = 0;
  {
    const int qseg = ((nrun + kRingThreads - 1) / kRingThreads) * 64, q0 = wave * qseg;
    u64 kreg[kTrips], hm[kTrips];
    unsigned carry = q0 > 0 && q0 - 1 < nrun ? (unsigned)(K2[q0 - 1] >> 32) : 0xffffffffu;   // (no voxel has that index: idx <= INT_MAX)
    int mine = 0;
#pragma unroll
    for (int it = 0; it < kTrips; it++) {
      kreg[it] = 0ull; hm[it] = 0ull;
      if (it * 64 < qseg) {
        const int t = q0 + it * 64 + lane;
        const u64 k0 = t < nrun ? K2[t] : ~0ull;
        const unsigned vid = (unsigned)(k0 >> 32);
        unsigned pv = (unsigned)__shfl_up((int)vid, 1);
        if (lane == 0) pv = carry;
        carry = (unsigned)__builtin_amdgcn_readlane((int)vid, 63);
        kreg[it] = k0;
        hm[it] = __ballot(t < nrun && vid != pv);
        mine += __popcll(hm[it]);
      }
    }
    int* s_vox = scan_tmp + 72;   // [8]
    if (lane == 0) s_vox[wave] = mine;
    __syncthreads();
    int running = 0;
    for (int w = 0; w < kRingThreads / 64; w++) { const int c = s_vox[w]; running += w < wave ? c : 0; nvox += c; }
#pragma unroll
    for (int it = 0; it < kTrips; it++) {
      if (it * 64 < qseg) {
        const int t = q0 + it * 64 + lane;
        if ((hm[it] >> lane) & 1ull) {
          const unsigned vid = (unsigned)(kreg[it] >> 32);
          float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;  // CentroidPoint<PointXYZI>: f32 sums in input order
          int npt = 0;
          u64 k = kreg[it];
          for (int u = t;;) {
            const int l0 = (int)((k >> 12) & 0xfffu), l1 = (int)(k & 0xfffu);
            for (int l = l0; l <= l1; l++) { sx += px[l]; sy += py[l]; sz += pz[l]; si += pi[l]; }
            npt += l1 - l0 + 1;
            if (++u >= nrun) break;
            k = K2[u];
            if ((unsigned)(k >> 32) != vid) break;
          }
          const float cnt = (float)npt;
          out[running + __popcll(hm[it] & ((1ull << lane) - 1ull))] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
        }
        running += __popcll(hm[it]);
      }
    }
  }
  if (tid == 0) S->ring_ds_cnt[r] = nvox;
  SR_STAMP();
  if (dbg_cyc && tid == 0) {
    for (int q = 0; q < 7; q++) dbg_cyc[r * 8 + q] = q + 1 < nstamp ? tstamp[q + 1] - tstamp[q] : 0;
    dbg_cyc[r * 8 + 7] = (long long)nrun | ((long long)nvox << 16) | ((long long)len << 32) | ((long long)ncand << 48);
  }
#undef SR_STAMP
  };
  // ONE call site: a second copy of the ring body costs the small tier 50 VGPRs, i.e. its second workgroup per CU.
  if constexpr (!BIG_TIER) one_ring((int)blockIdx.x);   // (straight-line: a loop around the body costs this tier as much)
  else sr_for_rings(S, kRingCapSmall, one_ring);        // one workgroup per ring, or the catch-all behind the small tier
}

template __global__ void k_sr_ring<kRingCapSmall, kSectCapSmall, false>(const float4* __restrict__, FrameScalars*, int* __restrict__, int* __restrict__,
                                                                       int* __restrict__, float4* __restrict__, float* __restrict__, int* __restrict__,
                                                                       int* __restrict__, int* __restrict__, long long* __restrict__, int*, int, size_t);
template __global__ void k_sr_ring<kMaxRingLen, kSectCap, true>(const float4* __restrict__, FrameScalars*, int* __restrict__, int* __restrict__,
                                                               int* __restrict__, float4* __restrict__, float* __restrict__, int* __restrict__,
                                                               int* __restrict__, int* __restrict__, long long* __restrict__, int*, int, size_t);

}  // namespace vloam
