// solve_dispatch.hip — the solve-method dispatchers of the ICP loop (host only): one frame
// (imls_register_frame, imls_solve*) and all frames of a batch (imls_register_frames).
#include "solve.h"

namespace imlsgpu {

void launch_solve(hipStream_t s, const SolveLaunch& L) {
    switch (L.kp.solve_method) {
        case IMLS_SOLVE_ROBUST: launch_solve_robust(s, L); break;
        case IMLS_SOLVE_RANSAC: launch_ransac(s, L); break;
        case IMLS_SOLVE_DRPM: launch_drpm_alone(s, L); break;
        default: {   // LS, weighted LS
            SolveState st = L.st;
            launch_solve_chain(s, L.N, L.blocks1, L.kp, L.cs, L.cd, L.cn, L.rows_d, L.weights, st, L.tr, L.update_pose,
                               L.rows_are_double, L.count);
        }
    }
}

int launch_solve_frames(hipStream_t s, const PairDev* tab, const int* n_host, int npairs, const KParams& kp,
                        const RansacParams& rp, int it) {
    switch (kp.solve_method) {
        case IMLS_SOLVE_RANSAC: return launch_ransac_batch(s, tab, n_host, npairs, kp, rp, it);
        case IMLS_SOLVE_ROBUST: launch_solve_robust_batch(s, tab, n_host, npairs, kp, it); break;
        default: launch_solve_batch(s, tab, n_host, npairs, kp, it);
    }
    return 0;
}

}  // namespace imlsgpu
