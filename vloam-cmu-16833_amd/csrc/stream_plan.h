// Which HIP priority each stream of a handle is created with, so that the stages that bound the sweep period get hardware queues of their
// own whatever GPU_MAX_HW_QUEUES the host process runs with.  Pure (budget, handle kind) -> plan: no HIP, compiled on its own by the CPU test.
//
// How the runtime deals queues (measured, profiles/r07_hw_queue_map.txt): a stream gets its hardware queue when it is CREATED, from the
// pool of its priority level — low, normal and high each keep a pool of up to GPU_MAX_HW_QUEUES queues.  While a pool has fewer, a new
// stream opens a new queue; once it is full, the stream shares the least-used queue of that pool (ties: the latest opened).  The process's
// null stream holds a queue of the normal pool.  Two streams on one queue run in single file, and a barrier packet (hipStreamWaitEvent on an
// event that has not fired yet) at the head of the queue holds back the other stream as well.
//
// Two plans:
//   FLAT   (the budget holds the null stream, every stream of the handle and kHostReserve streams of the host): every stream at normal
//          priority and the copy stream of host sweeps created (and used once) before the stage streams, as before the plan existed.
//   POOLED (anything smaller, e.g. the runtime's default of 4): one stage per priority level — scan registration (+ its VoxelGrid, + the
//          copy stream of host sweeps) low, odometry (+ images) normal, mapping high — so that no two of SR / LO / mapping can ever share a
//          queue, however many normal-priority streams the host holds.  The VoxelGrid's live wait for the scan registration sits on a queue of
//          the low pool: its own, or SR's once that pool is full (budget 1, or several handles alive), where it is behind the SR work it waits
//          for anyway.  The copy stream is created by the handle's first deferred host sweep, so device-pointer callers never open it; in the
//          low pool, host-fed sweeps from pageable memory ran at 0.92 x the device-resident rate, in the high pool at 0.60 x, and created first
//          it slowed every later handle of the process to ~2 500 scans/s.  The image stream in the normal pool: the coupled image loop at
//          2 800 - 2 900 frames/s (high pool: 1 950 - 2 260), batched image frames at 2 900 - 3 000 (high pool: 4 600 - 5 200; parent at 4
//          queues: 2 700 - 2 800 and 4 300 - 4 400; profiles/r07_hw_queue_map.txt).
// What is NOT promised: with several handles alive in one process the pools fill up and their stages share queues across handles (at budget
// 4: from the third handle on); in the flat plan, a host holding more than kHostReserve streams of its own pushes stages onto shared queues.
// Priorities do not change a single sequence's rate at 16 queues (profiles/r03_stream_priority_ab.txt); they only order the dispatch of
// workgroups when several queues have work ready.
#pragma once
#include <cstdlib>

namespace vloam_plan {

enum Pool { kNormal = 0, kHigh = 1, kLow = 2, kPools = 3 };
enum Stream { kSR = 0, kLO, kMap, kDS, kImg, kCopy, kStreams };

constexpr int kHostReserve = 4;   // normal-pool queues left to the host's own streams (profiles/r05_hw_queues.txt: 8 queues, four host streams)

// GPU_MAX_HW_QUEUES as the runtime reads it; unset (or not a positive number) is the runtime's default of 4
inline int budget_from_env(const char* v) {
  const int q = v ? atoi(v) : 0;
  return q >= 1 ? q : 4;
}

struct Plan {
  bool pooled = false;
  bool used[kStreams] = {};   // the handle has this stream (kCopy: planned for every handle, created by the first deferred host sweep)
  int pool[kStreams] = {};
  bool copy_first = false;    // vloam_create creates and warms the copy stream before the stage streams (else: the first deferred host sweep)
};

inline Plan make_plan(int budget, bool mapping, bool image) {
  Plan p;
  p.used[kSR] = p.used[kLO] = p.used[kCopy] = true;
  p.used[kMap] = p.used[kDS] = mapping;
  p.used[kImg] = image;
  int n = 0;
  for (int s = 0; s < kStreams; s++) n += p.used[s];
  p.pooled = 1 + n + kHostReserve > budget;
  p.copy_first = !p.pooled;
  if (!p.pooled) return p;   // all kNormal
  p.pool[kSR] = kLow;
  p.pool[kDS] = kLow;
  p.pool[kLO] = kNormal;
  p.pool[kMap] = kHigh;
  p.pool[kImg] = kNormal;
  p.pool[kCopy] = kLow;
  return p;
}

}  // namespace vloam_plan
