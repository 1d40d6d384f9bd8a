// The unified step launch's workgroup rows (see steptail.h).
#include <vector>

#include "steptail.h"

namespace cmamd {

// The rows' order, one of two (the measurements: DESIGN.md section 5's tables
// and profiles/r05_schedules.txt):
//   * chi^2 rows present (ng > 0): chi^2, quadratic form, pass, Metropolis.
//     The Metropolis rows wait for both tails, so the tails are dispatched
//     first; the pass ahead of the quadratic form measured 58.4 against
//     40.9 us/step (round 4), the Metropolis rows earlier 61-94 against 38.5
//     (round 5).
//   * chi^2 folded into the Metropolis workgroups (ng == 0): Metropolis,
//     quadratic form, pass.  They then wait resident for their tiles'
//     producers (64 of the launch's >= 512 slots) and compute the chi^2 while
//     the quadratic form runs: 32.6-32.7 us a middle launch against 41.0 with
//     the Metropolis rows last and 33.6-33.8 with the chi^2 as rows (round 6).
std::vector<int2> tail_rows(int nq, int ng, int np, int nm) {
    std::vector<int2> rows;
    auto emit = [&](int role, int n) {
        for (int k = 0; k < (n + 7) / 8; k++) rows.push_back(int2{role, k});
    };
    if (ng > 0) {
        emit(TAIL_GAUSS, ng);
        emit(TAIL_QF, nq);
        emit(TAIL_PASS, np);
        emit(TAIL_MH, nm);
    } else {
        emit(TAIL_MH, nm);
        emit(TAIL_QF, nq);
        emit(TAIL_PASS, np);
    }
    return rows;
}

}  // namespace cmamd
