// pos_tiling.h — the whole-position tiling table of k_conv_pos (conv_kernels.hip) and k_tower (tower_kernels.hip); host only.
#pragma once
#include <hip/hip_runtime.h>

namespace tg {

// Whole-position tilings of k_conv_pos and k_tower: RTW row tiles per wave, NWAVES waves, PW positions and CTW channel tiles per
// workgroup, for the table of N×N boards with F channels.  A workgroup's run time is that of its positions' row tiles, whatever the
// batch: with 16 positions per workgroup a 32-position call (the reference's BATCH_SIZE) ran 2 workgroups for as long as 4096
// positions take.  Small batches therefore take fewer positions per workgroup; the per-element arithmetic — taps, chunks, MFMA
// k-steps in the same order — does not depend on the tiling, so results are bit-identical.
template <int N_, int F_, int RTW_, int NWAVES_, int PW_, int CTW_>
struct PosTiling {
    static constexpr int N = N_, F = F_, RTW = RTW_, NWAVES = NWAVES_, PW = PW_, CTW = CTW_;
};

// launch(PosTiling<…>{}) for B positions of the (n, F) table: 5×5 with 64 or 128, 6×6 with 128
template <class Launch>
static hipError_t launch_pos_tiled(int n, int F, int B, Launch&& launch) {
    if (n == 5 && F == 64) {  // 16 positions = 25 row tiles, 4 channel tiles × 2 row groups of 13
        // (round 6, measured at 300 … 2048 positions with 1 / 2 / 4 / 8 positions per workgroup: these brackets are within 11 % of the
        // best choice everywhere — two co-resident workgroups of half the size take as long as one; eight waves instead of four: 5 %;
        // every layer streaming the same L2-hot weights: no difference — profiles/r06_e_tower_pw_sweep.txt)
        if (B <= 256) return launch(PosTiling<5, 64, 2, 4, 1, 4>{});
        if (B <= 512) return launch(PosTiling<5, 64, 4, 4, 2, 4>{});
        if (B <= 1024) return launch(PosTiling<5, 64, 7, 4, 4, 4>{});
        if (B <= 2048) return launch(PosTiling<5, 64, 13, 4, 8, 4>{});
        return launch(PosTiling<5, 64, 13, 8, 16, 4>{});
    }
    if (n == 6 && F == 128) {  // 4 positions = 9 row tiles, 8 channel tiles
        if (B <= 256) return launch(PosTiling<6, 128, 3, 8, 1, 8>{});
        if (B <= 512) return launch(PosTiling<6, 128, 5, 8, 2, 8>{});
        return launch(PosTiling<6, 128, 9, 8, 4, 8>{});
    }
    if (n == 5 && F == 128) {  // 8 positions = 200 rows in 13 row tiles, 8 channel tiles
        if (B <= 256) return launch(PosTiling<5, 128, 2, 8, 1, 8>{});
        if (B <= 512) return launch(PosTiling<5, 128, 4, 8, 2, 8>{});
        if (B <= 1024) return launch(PosTiling<5, 128, 7, 8, 4, 8>{});
        return launch(PosTiling<5, 128, 13, 8, 8, 8>{});
    }
    return hipErrorInvalidValue;
}

}  // namespace tg
