// engine.h — internal definition of the opaque TgEngine handle (host side of libtakgpu.so)
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/takgpu.h"
#include "board.cuh"

namespace tg {

void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define TG_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return tg::fail(TG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

// RAII device allocation
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t ensure(size_t nbytes) {
        if (nbytes <= bytes) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, nbytes);
        if (e == hipSuccess) bytes = nbytes;
        return e;
    }
    template <class T>
    T* as() const { return (T*)p; }
};
// `b` sized for `count` elements of the field it is bound to: the field's declared type is the one statement of the element size
template <class T>
hipError_t bind(DevBuf& b, T*& field, size_t count) {
    hipError_t e = b.ensure(count * sizeof(T));
    field = b.as<T>();
    return e;
}

struct Net;     // net.hip
struct Search;  // search_host.h
struct Trainer; // train.hip
struct Window;  // window.hip
struct Solver;  // solve.hip
struct WindowDev;  // kernels.h
struct SearchDev;  // search.cuh

}  // namespace tg

struct TgEngine {
    TgConfig cfg;
    tg::Geom g;
    hipStream_t stream = nullptr;
    int cin = 0;          // input channels
    int cin_pad = 0;      // channels per NHWC input row (multiple of 16, zero padded)
    int policy_size = 0;  // P
    bool legacy5 = false; // FC5 head → legacy 1575 LUT indices
    tg::DevBuf lut5;      // int16[25*4*32]
    // host-API scratch (sized for cfg.max_batch items)
    tg::DevBuf s_states, s_moves, s_counts, s_status, s_planes, s_policy, s_eval, s_index;
    tg::Net* net = nullptr;
    tg::Search* search = nullptr;
    tg::Trainer* trainer = nullptr;
    tg::Window* window = nullptr;  // the example window: outlives searches, self-play drivers and trainers, dies with the engine
    // dihedral symmetries (symm.hip): the policy permutation tables int32[8][P] built at tg_net_finalize, tg_policy_eval_symm's
    // staging (the caller's states; the folded outputs), the search's mode (TgSearchSymmetry) and its count of transformed leaves
    tg::DevBuf symm_perm, symm_src, symm_policy, symm_eval, symm_count;
    int symm_mode = 0;
    tg::Solver* solver = nullptr;  // forced-win solver scratch (tg_solve / tg_search_solve): created at the first call, dies with the engine
    ~TgEngine();
};

namespace tg {
// engine.hip: host-side sanity check of caller-supplied packed states (TG_ERR_INVALID_ARG naming the first bad one)
int validate_states(const TgEngine* e, int k, const uint8_t* states, const char* who);
// net.hip
int net_create(TgEngine* e);
void net_destroy(Net* n);
// search.hip
void search_destroy(Search* s);
int search_poll_errors(TgEngine* e);  // after a stream sync: device error flags → status
int net_poll_errors(TgEngine* e);     // after a stream sync: the network kernels' error word → status
int net_set_tensor(TgEngine* e, const char* name, const float* data, size_t count);
int net_finalize(TgEngine* e);
bool net_ready(const TgEngine* e);
// forward on device: planes NHWC (n × nsq × C) → policy (n × P, softmax) and eval (n)
int net_forward_dev(TgEngine* e, int n, const float* d_planes_nhwc, float* d_policy, float* d_eval);
// same from packed states (device); encodes inside the fused tower when the topology allows, else via k_encode
int net_forward_states_dev(TgEngine* e, int n, const uint8_t* d_states, float* d_policy, float* d_eval);
bool net_takes_states(const TgEngine* e);  // true when the fused tower encodes in-kernel
struct FcGatherArgs;  // kernels.h
const float* net_fc_stats(const TgEngine* e, int* blocks, int* stride);  // block-wise softmax statistics that go with net_fc_logits' buffer ([batch][stride][2]), or nullptr
bool net_gather_ok(const TgEngine* e, int leaves);          // will a logits-only forward of `leaves` rows write the children's logits (net_set_gather)?
void net_set_gather(TgEngine* e, const FcGatherArgs* g);    // the search's child_pidx / leaf_rec / child_logit buffers, or nullptr
const float* net_fc_logits(const TgEngine* e, int* ld);  // FC head: logits buffer for logits-only forwards (d_policy = nullptr), else nullptr
const std::map<std::string, std::vector<float>>* net_tensors(const TgEngine* e);  // tensors as given to tg_net_set_tensor
// train.hip
void trainer_destroy(Trainer* t);
// the complete host-side check of example `s` of the caller's arrays (tg_train_chunk, tg_train, tg_window_push): TG_ERR_INVALID_ARG naming it
int validate_example(const TgEngine* e, int s, const uint8_t* states, const int32_t* n_moves, const uint32_t* visits);
// Network::train on `count` rows of the example window, logical offset j at window row (row0 + j) % capacity (tg_window_train)
int train_window(TgEngine* e, const WindowDev& W, uint32_t row0, int count, uint64_t seed, float* mean_loss_p, float* mean_loss_z,
                 int32_t* steps);
// window.hip
void window_destroy(Window* w);
// the device arrays of the engine's window and its host-side counters (reanalyse.hip); false: the engine has no window
bool window_view(const TgEngine* e, WindowDev* d, uint64_t* count, uint64_t* evicted);
// solve.hip
void solver_destroy(Solver* s);
// symm.hip
int symm_tables_build(TgEngine* e);  // (tg_net_finalize) the device tables behind tg_policy_eval_symm and TG_SYMM_HASHED, built once
// (search_iterate) the hashed image of the iteration's leaves, between the tree kernel and the forward; TG_SYMM_OFF: nothing
int symm_search_leaves(TgEngine* e, const SearchDev& d, int leaves);
int symm_search_prepare(TgEngine* e);  // the engine's mode onto its search: a search fed by planes is fed by packed leaf states instead
}  // namespace tg
