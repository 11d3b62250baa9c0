// tree_launch.h — host-side launch helpers of the tree kernels, shared by search_kernels.hip and search_list_kernels.hip
// (included behind tree_pass.cuh, whose WPB they use)
#pragma once

namespace tg {

static inline dim3 wgrid(int waves) { return dim3((waves + WPB - 1) / WPB); }

// the tree kernels are compiled for the board sizes of the BASELINE configs (n as a constant) and once for any size (3×3, 4×4);
// one wave per game: WAVES = S.G, or the length of a compacted list
#define TG_BY_BOARD(KERNEL, WAVES, ...)                                                                     \
    do {                                                                                                    \
        if (S.n == 5) hipLaunchKernelGGL(KERNEL<5>, wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__);      \
        else if (S.n == 6) hipLaunchKernelGGL(KERNEL<6>, wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL<0>, wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__);               \
    } while (0)

}  // namespace tg
