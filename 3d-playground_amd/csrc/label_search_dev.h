// The annotator's coarse-to-fine search of a box centre, shared by label_rebase.hip (Annotator.replace_homgraphy, fp64) and
// label_assist.hip (Annotator.paste_in_2D_bbox, fp32): per round a grid x grid window of candidate centres around the current one,
// torch.argmin of their errors, and the winner starts the next round.
#pragma once
#include <math.h>

#include "wave_dev.h"

// One wave searches one box; every lane calls with the same arguments and gets the same results.  score(x, y) -> T is the error of
// the candidate centre (x, y).  Per round r the window is centre +- (T)radii[r], its axes are np.linspace(.., grid) in T, the lanes
// take candidates l, l + 64, ... in ascending order (index = ix * grid + iy) and a wave reduction on (error, index) picks the first
// smallest as torch.argmin does; lane 0 writes the winner's index to idx_row[r].  Every operation is in T: nothing is promoted.
// Returns true with the last winner in (cx, cy) and its error in err.  A round whose minimum is not finite sets RN_LABEL_BAD_ERROR
// in *status, puts -1 back into the indices of the rounds before it and returns false: the caller leaves the box out (wave-uniform).
template <typename T, class Score>
__device__ __forceinline__ bool label_grid_search(T &cx, T &cy, T &err, const double *__restrict__ radii, int rounds, int grid,
                                                  int32_t *__restrict__ idx_row, int32_t *status, Score score) {
    const int lane = threadIdx.x & (RN_WAVE - 1);
    const int cells = grid * grid;
    const torch_argmin_before<T> before;
    for (int r = 0; r < rounds; ++r) {
        const T rad = (T)radii[r];
        const T x0 = cx - rad, x1 = cx + rad, y0 = cy - rad, y1 = cy + rad;
        const T sx = (x1 - x0) / (T)(grid - 1), sy = (y1 - y0) / (T)(grid - 1);
        T best = INFINITY;
        int best_i = RN_NO_INDEX;
        for (int c = lane; c < cells; c += RN_WAVE) {                           // ascending per lane
            const T e = score(rn_linspace<T>(x0, x1, sx, c / grid, grid), rn_linspace<T>(y0, y1, sy, c % grid, grid));
            if (before(e, c, best, best_i)) { best = e; best_i = c; }
        }
        wave_arg_first(best, best_i, before);                                   // a total order: all lanes agree
        if (!isfinite(best) || best_i >= cells) {                               // wave-uniform
            if (lane == 0) {
                rn_flag(status, RN_LABEL_BAD_ERROR);
                for (int q = 0; q < r; ++q) idx_row[q] = -1;                    // the box is left out as a whole
            }
            return false;
        }
        cx = rn_linspace<T>(x0, x1, sx, best_i / grid, grid);
        cy = rn_linspace<T>(y0, y1, sy, best_i % grid, grid);
        err = best;
        if (lane == 0) idx_row[r] = best_i;
    }
    return true;
}
