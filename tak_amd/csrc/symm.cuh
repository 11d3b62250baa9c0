// symm.cuh — the dihedral image of a wave-resident position and of a move code (Symmetry, tak/src/symm.rs:11-20; board.cuh
// sym_apply / sym_apply_inverse / sym_dir). move_symm_image is the one statement of the move transform: k_augment,
// k_example_metrics and k_symm_perm call it. ws_symm_image serves symm_kernels.hip; k_augment and k_eval_images keep the same
// lines inline, because calling it there reorders two instructions of each and those kernels stay as they were.
#pragma once
#include "board.cuh"

namespace tg {

// s under symmetry sym: the square this lane ends up holding comes from its pre-image (header fields do not move)
__device__ inline WState ws_symm_image(const WState& s, const Geom& g, int sym) {
    const int lane = lane_id();
    int col = lane % g.n, row = lane / g.n;
    sym_apply_inverse(g.n, sym, col, row);
    const int src = lane < g.nsq ? row * g.n + col : lane;
    WState t = s;
    t.stack = shfl64(s.stack, src);
    t.height = (uint32_t)__shfl((int)s.height, src);
    t.top = (uint32_t)__shfl((int)s.top, src);
    return t;
}

// the move code of m's image under sym (the square follows sym_apply, a spread's direction sym_dir; a placement's piece stays)
__device__ inline uint32_t move_symm_image(uint32_t m, int n, int sym) {
    int c = (int)(m & 63u) % n, r = (int)(m & 63u) / n;
    sym_apply(n, sym, c, r);
    uint32_t pat = m >> 8, f = (m >> 6) & 3u;
    if (pat) f = sym_dir(sym, f);
    return (uint32_t)(r * n + c) | (f << 6) | (pat << 8);
}

}  // namespace tg
