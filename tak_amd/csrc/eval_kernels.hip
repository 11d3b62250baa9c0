// eval_kernels.hip — losses of the INFERENCE network on examples (tg_eval_examples): the kernels behind the forward.
// No counterpart in the reference, which prints the training losses of network.rs:86 only.
//   k_eval_images     the dihedral image of an example's state (the augmentation's transform, no policy target);
//   k_example_metrics one wave per position: log-softmax statistics of the full logits row, then the example's sparse
//                     (move, visits) list through move_index — policy cross-entropy, target entropy, the two arg-maxes,
//                     (z − v)² — into one 4-float row (+ the target entropy, which no row carries);
//   k_eval_sum        adds a slice's rows to the call's sums in f64, in position order.
#include "board.cuh"
#include "kernels.h"
#include "softmax.cuh"
#include "symm.cuh"

namespace tg {

constexpr int EVAL_WAVES = 4;  // positions per 256-thread block

// position q of a slice (q = phase + wave index when symmetries are on: the slice may start inside an example's 8 images)
__device__ inline void eval_position(int w, int phase, int symm, int& ex, int& sym) {
    const int q = phase + w;
    ex = symm ? q >> 3 : w;
    sym = symm ? q & 7 : 0;
}

// states[ex] under symmetry sym → out[w]; the transform of k_augment (the lane's square comes from its pre-image)
__global__ __launch_bounds__(256) void k_eval_images(const uint8_t* __restrict__ states, int count, int phase, int n,
                                                     uint8_t* __restrict__ out) {
    const int w = (int)(blockIdx.x * EVAL_WAVES + (threadIdx.x >> 6));
    if (w >= count) return;
    int ex, sym;
    eval_position(w, phase, 1, ex, sym);
    const int lane = lane_id();
    const Geom g = make_geom(n);
    WState s;
    ws_load(s, states + (size_t)ex * g.bytes, g);
    // (symm.cuh ws_symm_image is these lines; calling it here reorders two instructions of this kernel, which is kept as it was)
    int col = lane % n, row = lane / n;
    sym_apply_inverse(n, sym, col, row);
    const int src = lane < g.nsq ? row * n + col : lane;
    WState t = s;
    t.stack = shfl64(s.stack, src);
    t.height = (uint32_t)__shfl((int)s.height, src);
    t.top = (uint32_t)__shfl((int)s.top, src);
    ws_store(t, out + (size_t)w * g.bytes, g);
}

// first maximum in list order: the larger key wins, on equal keys the smaller list index
template <class K>
__device__ inline void first_max_wave(K& key, int& idx) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const K ok = __shfl_xor(key, d);
        const int oi = __shfl_xor(idx, d);
        if (oi >= 0 && (idx < 0 || ok > key || (ok == key && oi < idx))) { key = ok; idx = oi; }
    }
}

// Logits of one position as R rows of `cs` floats with C valid columns: the FC head is one row of ld floats with P valid
// (column P, the value pre-activation, is NOT one of them); the conv head is nsq rows of cout_pad channels with P / nsq valid.
// Policy index p sits at (p % R)·cs + p / R.
// ex_rec[ex] = {first entry of the example's moves / visits in the packed lists, n_moves, result bits, 0}.
// eval: tanh of the value head as the forward wrote it, or nullptr = tanh(logit P) of the FC row (what k_softmax_stats writes).
__global__ __launch_bounds__(256) void k_example_metrics(const float* __restrict__ logits, size_t pos_stride, int R, int cs, int C,
                                                         const float* __restrict__ eval, const int4* __restrict__ ex_rec,
                                                         const uint16_t* __restrict__ moves, const uint32_t* __restrict__ visits,
                                                         int count, int phase, int symm, int n, int legacy5,
                                                         const int16_t* __restrict__ lut5, float* __restrict__ rows,
                                                         float* __restrict__ entropy) {
    const int w = (int)(blockIdx.x * EVAL_WAVES + (threadIdx.x >> 6));
    if (w >= count) return;
    const int lane = lane_id();
    int ex, sym;
    eval_position(w, phase, symm, ex, sym);
    const float* x = logits + (size_t)w * pos_stride;
    // ---- log Σ exp over the valid logits: two passes over the row (the second one hits L2), 16 bytes per lane and step
    const int n4 = (R * cs) >> 2;
    const softmax_f32x4* x4 = (const softmax_f32x4*)x;
    float mx = -INFINITY;
    for (int i = lane; i < n4; i += 64) {
        const softmax_f32x4 v = x4[i];
        const int c = (4 * i) % cs;
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (c + t < C) mx = fmaxf(mx, v[t]);
    }
    mx = wave_max(mx);
    float se = 0.0f;
    for (int i = lane; i < n4; i += 64) {
        const softmax_f32x4 v = x4[i];
        const int c = (4 * i) % cs;
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (c + t < C) se += expf(v[t] - mx);
    }
    se = wave_sum(se);
    const float lse = mx + logf(se);
    // ---- the example's listed moves: ≤ TG_MAX_MOVES = 8 per lane, list entry k = lane + 64 j
    const int4 rec = ex_rec[ex];
    const int nm = rec.y;
    const float z = __int_as_float(rec.z);
    const uint16_t* mv = moves + rec.x;
    const uint32_t* vs = visits + rec.x;
    uint32_t part = 0;
    for (int k = lane; k < nm; k += 64) part += vs[k];
    for (int d = 32; d >= 1; d >>= 1) part += (uint32_t)__shfl_xor((int)part, d);
    const float total = (float)part;  // (the training target's own division: k_augment)
    float lp = 0.0f, ent = 0.0f;
    uint32_t best_v = 0;
    int best_vk = -1;
    float best_l = -INFINITY;
    int best_lk = -1;
    for (int k = lane; k < nm; k += 64) {
        const uint32_t tm = move_symm_image(mv[k], n, sym);
        const int idx = move_index_dev(tm, n, legacy5 != 0, lut5);
        const bool ok = idx >= 0 && idx < R * C;
        const float l = ok ? x[(size_t)(idx % R) * cs + idx / R] : -INFINITY;
        const uint32_t v = vs[k];
        if (v && ok) {
            const float pi = (float)v / total;
            lp += pi * (l - lse);
            ent += pi * logf(pi);
        }
        if (best_vk < 0 || v > best_v) { best_v = v; best_vk = k; }
        if (best_lk < 0 || l > best_l) { best_l = l; best_lk = k; }
    }
    lp = wave_sum(lp);
    ent = wave_sum(ent);
    first_max_wave(best_v, best_vk);
    first_max_wave(best_l, best_lk);
    if (lane == 0) {
        const float v = eval ? eval[w] : tanhf(x[C]);
        const float dz = z - v;
        *(float4*)&rows[(size_t)w * 4] = make_float4(-lp, dz * dz, best_lk == best_vk ? 1.0f : 0.0f, v);
        entropy[w] = -ent;
    }
}

// acc = {Σ loss_p, Σ loss_z, Σ target entropy} as doubles, then {top1, sign_ok, decided} as uint64: this slice's positions are
// added behind what the earlier slices of the call left there, one after the other, so the f64 sums are those of ONE pass over
// the call's positions in order whatever the slicing.  One wave: 64 rows are fetched together and parked in LDS, lanes 0..2
// then add one column each, row by row.
__global__ __launch_bounds__(64) void k_eval_sum(const float* __restrict__ rows, const float* __restrict__ entropy,
                                                 const int4* __restrict__ ex_rec, int count, int phase, int symm,
                                                 double* __restrict__ acc) {
    __shared__ float col[3][64];
    const int lane = (int)threadIdx.x;
    double s = lane < 3 ? acc[lane] : 0.0;
    unsigned long long top1 = 0, sign_ok = 0, decided = 0;
    for (int w0 = 0; w0 < count; w0 += 64) {
        const int w = w0 + lane;
        if (w < count) {
            const float4 r = *(const float4*)&rows[(size_t)w * 4];
            int ex, sym;
            eval_position(w, phase, symm, ex, sym);
            const float z = __int_as_float(ex_rec[ex].z);
            col[0][lane] = r.x;
            col[1][lane] = r.y;
            col[2][lane] = entropy[w];
            top1 += r.z != 0.0f;
            decided += z != 0.0f;
            sign_ok += z != 0.0f && r.w * z > 0.0f;
        }
        __syncthreads();  // (a one-wave block)
        const int m = min(64, count - w0);
        const float* mine = col[lane < 3 ? lane : 0];
        for (int j = 0; j < m; j++) s += (double)mine[j];
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) {
        top1 += __shfl_xor(top1, d);
        sign_ok += __shfl_xor(sign_ok, d);
        decided += __shfl_xor(decided, d);
    }
    if (lane < 3) acc[lane] = s;
    if (lane == 0) {
        unsigned long long* cnt = (unsigned long long*)(acc + 3);
        cnt[0] += top1;
        cnt[1] += sign_ok;
        cnt[2] += decided;
    }
}

// ---- launchers --------------------------------------------------------------------------------
void launch_eval_images(hipStream_t st, const uint8_t* states, int count, int phase, int n, uint8_t* out) {
    if (count > 0) hipLaunchKernelGGL(k_eval_images, dim3((count + EVAL_WAVES - 1) / EVAL_WAVES), dim3(256), 0, st, states, count, phase, n, out);
}

hipError_t launch_example_metrics(hipStream_t st, const EvalLogits& L, const int4* ex_rec, const uint16_t* moves, const uint32_t* visits,
                                  int count, int phase, bool symm, int n, bool legacy5, const int16_t* lut5, float* rows, float* entropy) {
    if (count <= 0) return hipSuccess;
    // 16-byte loads over whole rows; the value column must exist where the kernel is asked to read it
    if (L.R <= 0 || (L.cs & 3) || L.C > L.cs || (L.pos_stride & 3) || (!L.eval && (L.R != 1 || L.C >= L.cs))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_example_metrics, dim3((count + EVAL_WAVES - 1) / EVAL_WAVES), dim3(256), 0, st, L.logits, L.pos_stride, L.R, L.cs, L.C,
                       L.eval, ex_rec, moves, visits, count, phase, symm ? 1 : 0, n, legacy5 ? 1 : 0, lut5, rows, entropy);
    return hipGetLastError();
}

hipError_t launch_eval_sum(hipStream_t st, const float* rows, const float* entropy, const int4* ex_rec, int count, int phase, bool symm,
                           double* acc) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_eval_sum, dim3(1), dim3(64), 0, st, rows, entropy, ex_rec, count, phase, symm ? 1 : 0, acc);
    return hipGetLastError();
}

}  // namespace tg
