// tower_stamps.cuh — the diagnostic build's phase stamps (TG_STAMP) of the fused towers, k_conv_halo and k_fc_ring (TG_FC_STAMP).
// One definition of g_tower_stamps per translation unit: a probe that #includes two of the kernel units gets one.  Compile at most ONE
// unit of a library with -DTG_TOWER_STAMPS (scripts/probes/fc_ring_probe.sh's UNIT): two would each define the host-side symbol.
#pragma once
#include <hip/hip_runtime.h>

namespace tg {

// Diagnostic build only (scripts/probes/tower_stamps.hip, -DTG_TOWER_STAMPS): s_memtime stamps of workgroup 0's waves at
// the phase boundaries of every layer, written to a buffer nothing else reads.  The product build compiles none of it.
#ifdef TG_TOWER_STAMPS
__device__ unsigned long long* g_tower_stamps = nullptr;  // [layer][wave][8]
#define TG_STAMP(layer, slot)                                                                                       \
    do {                                                                                                            \
        if (blockIdx.x == 0 && g_tower_stamps && (threadIdx.x & 63) == 0)                                           \
            g_tower_stamps[((size_t)(layer) * 16 + (threadIdx.x >> 6)) * 8 + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define TG_STAMP(layer, slot) do { } while (0)
#endif

}  // namespace tg
