// Test program: the stream plan of a handle (csrc/stream_plan.h), compiled on its own (no HIP).  For every budget 1..32, handle kind and
// number of normal-pool queues the host holds before the handle (its null stream and 0..5 more), one line:
//   "<budget> <mapping> <image> <host_normal> <pooled> <copy_first> <pool[6]> <queue[6]>"   (streams: SR LO map ds img copy; -1 = unused)
// The queues come from a model of the HIP runtime's placement rule as stream_plan.h states it and profiles/r07_hw_queue_map.txt measured it
// (tools/queue_probe.hip): a stream gets a new queue of its priority level's pool while that pool holds fewer than `budget`, else the
// least-used queue of the pool, the latest opened among equals.  The model is this test's, not the library's: it checks the plan against the
// rule, it cannot check the rule against the runtime.
#include <cstdio>
#include <cstdlib>
#include "stream_plan.h"

using namespace vloam_plan;

// queue = pool * 1000 + index in the pool; streams created in vloam_create's order (the copy stream first with copy_first, last without)
static void predict_queues(const Plan& p, int budget, int host_normal, int queue[kStreams]) {
  int refs[kPools][64] = {};
  int open[kPools] = {};
  for (int k = 0; k < host_normal && k < budget && k < 64; k++) refs[kNormal][open[kNormal]++] = 1;
  const int first[kStreams] = {kCopy, kSR, kLO, kMap, kDS, kImg}, last[kStreams] = {kSR, kLO, kMap, kDS, kImg, kCopy};
  const int* order = p.copy_first ? first : last;
  for (int s = 0; s < kStreams; s++) queue[s] = -1;
  for (int i = 0; i < kStreams; i++) {
    const int s = order[i];
    if (!p.used[s]) continue;
    const int pl = p.pool[s];
    int q = open[pl];
    if (open[pl] < budget && open[pl] < 64) {
      open[pl]++;
    } else {
      q = open[pl] - 1;
      for (int j = open[pl] - 1; j >= 0; j--) if (refs[pl][j] < refs[pl][q]) q = j;
    }
    refs[pl][q]++;
    queue[s] = pl * 1000 + q;
  }
}

int main() {
  if (budget_from_env(nullptr) != 4 || budget_from_env("") != 4 || budget_from_env("0") != 4 || budget_from_env("16") != 16) return 3;
  for (int budget = 1; budget <= 32; budget++)
    for (int mapping = 0; mapping < 2; mapping++)
      for (int image = 0; image < 2; image++)
        for (int host = 1; host <= 6; host++) {
          const Plan p = make_plan(budget, mapping != 0, image != 0);
          int q[kStreams];
          predict_queues(p, budget, host, q);
          std::printf("%d %d %d %d %d %d", budget, mapping, image, host, (int)p.pooled, (int)p.copy_first);
          for (int s = 0; s < kStreams; s++) std::printf(" %d", p.used[s] ? p.pool[s] : -1);
          for (int s = 0; s < kStreams; s++) std::printf(" %d", q[s]);
          std::printf("\n");
        }
  return 0;
}
