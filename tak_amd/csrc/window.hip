// window.hip — host side of the tg_window_* entry points of include/takgpu.h: the example window of training_loop
// (train/src/main.rs:26,56-123 — one Vec<Example> that every self-play round extends, `.data` files are loaded into, that is
// truncated to the latest MAX_EXAMPLES and trained on as a whole) as a ring of canonical example rows in device memory.
// Examples enter from the self-play ring (tg_window_absorb, k_window_absorb) or from the host (tg_window_push) and leave as training
// chunks (tg_window_train → train.hip's train_window, k_window_gather) or as a host copy (tg_window_read).
//
// The k-th example that entered since create / clear lives at row k % capacity (window.h), so with `entered` examples so far and
// count = min(entered, capacity) of them kept, logical index i (0 = oldest) is row (entered − count + i) % capacity.
#include <algorithm>
#include <cstring>

#include "search_host.h"
#include "window.h"

namespace tg {

struct Window {
    DevBuf states, n_moves, result, game_id, moves, visits;
    WindowDev d{};
    uint64_t capacity = 0, entered = 0;
    uint64_t count() const { return std::min(entered, capacity); }
    uint64_t evicted() const { return entered - count(); }
};

void window_destroy(Window* w) { delete w; }

bool window_view(const TgEngine* e, WindowDev* d, uint64_t* count, uint64_t* evicted) {
    if (!e || !e->window) return false;
    *d = e->window->d;
    *count = e->window->count();
    *evicted = e->window->evicted();
    return true;
}

namespace {

int need_window(TgEngine* e, const char* who) {
    if (!e) return fail(TG_ERR_INVALID_ARG, std::string(who) + ": null engine");
    hipError_t err = hipSetDevice(e->cfg.device);
    if (err != hipSuccess) return fail(TG_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(err));
    if (!e->window) return fail(TG_ERR_STATE, std::string(who) + ": the engine has no example window (tg_window_create)");
    return TG_OK;
}

// one array of the window ← / → the host, `n` rows of `row` bytes at cursor position `first`: at most two runs (window.h)
int copy_rows(TgEngine* e, const Window* w, void* d_base, void* host, size_t row, uint64_t first, uint64_t n, bool to_device) {
    const RingRuns r = ring_runs(first, n, w->capacity);
    for (int k = 0; k < r.count; k++) {
        uint8_t* dev = (uint8_t*)d_base + (size_t)r.start[k] * row;
        uint8_t* hst = (uint8_t*)host + (size_t)r.at[k] * row;
        const size_t bytes = (size_t)r.len[k] * row;
        if (to_device) TG_HIP(hipMemcpyAsync(dev, hst, bytes, hipMemcpyHostToDevice, e->stream));
        else TG_HIP(hipMemcpyAsync(hst, dev, bytes, hipMemcpyDeviceToHost, e->stream));
    }
    return TG_OK;
}

}  // namespace
}  // namespace tg

using namespace tg;

extern "C" {

int tg_window_create(TgEngine* e, int capacity) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "tg_window_create: null engine");
    if (capacity < 0) return fail(TG_ERR_INVALID_ARG, "tg_window_create: capacity must be positive, or 0 to free the window");
    const size_t sb = (size_t)e->g.bytes;
    const size_t widest = std::max(sb, (size_t)EX_MOVES * 4);  // the largest row of the six arrays
    if ((size_t)capacity > SIZE_MAX / widest)
        return fail(TG_ERR_INVALID_ARG, "tg_window_create: the byte size of " + std::to_string(capacity) + " examples overflows size_t");
    TG_HIP(hipSetDevice(e->cfg.device));
    if (e->window) {  // an absorb into the old one may still be running
        TG_HIP(hipStreamSynchronize(e->stream));
        window_destroy(e->window);
        e->window = nullptr;
    }
    if (capacity == 0) return TG_OK;
    std::unique_ptr<Window> w(new Window());
    const size_t C = (size_t)capacity;
    // (a failed allocation returns from here: `w` frees what it had got, and the engine is left without a window)
    TG_HIP(bind(w->states, w->d.states, C * sb));
    TG_HIP(bind(w->n_moves, w->d.n_moves, C));
    TG_HIP(bind(w->result, w->d.result, C));
    TG_HIP(bind(w->game_id, w->d.game_id, C));
    TG_HIP(bind(w->moves, w->d.moves, C * EX_MOVES));
    TG_HIP(bind(w->visits, w->d.visits, C * EX_MOVES));
    w->d.capacity = (uint32_t)capacity;
    w->d.bytes = (uint32_t)sb;
    w->capacity = C;
    e->window = w.release();
    return TG_OK;
}

int tg_window_info(TgEngine* e, TgWindowInfo* out) {
    int rc = need_window(e, "tg_window_info");
    if (rc) return rc;
    if (!out) return fail(TG_ERR_INVALID_ARG, "tg_window_info: null argument");
    const Window* w = e->window;
    out->capacity = w->capacity;
    out->count = w->count();
    out->entered = w->entered;
    out->evicted = w->evicted();
    return TG_OK;
}

int tg_window_clear(TgEngine* e) {
    int rc = need_window(e, "tg_window_clear");
    if (rc) return rc;
    e->window->entered = 0;  // rows are written before they are read: nothing to erase on the device
    return TG_OK;
}

int tg_window_absorb(TgEngine* e, int32_t* n_absorbed) {
    int rc = need_window(e, "tg_window_absorb");
    if (rc) return rc;
    if (!e->search || !e->search->selfplay) return fail(TG_ERR_STATE, "tg_window_absorb: tg_selfplay_create has not been called");
    Search* s = e->search;
    Window* w = e->window;
    rc = sync_and_check(e);  // the one wait, as tg_selfplay_drain: how many examples have finished
    if (rc) return rc;
    unsigned long long total = 0;
    TG_HIP(hipMemcpy(&total, s->p.stats + ST_EXAMPLES, 8, hipMemcpyDeviceToHost));
    const unsigned long long ME = (unsigned long long)s->p.max_examples;
    if (total - s->drained > ME) {  // older ones were overwritten in the ring: skipped, and counted (tg_selfplay_drain's rule)
        s->dropped += total - ME - s->drained;
        s->drained = total - ME;
    }
    const uint64_t k = total - s->drained;  // ≤ max_examples < 2^31
    // more than the window holds: the oldest never land (they count as entered and evicted), the newest `capacity` are copied
    const uint64_t skip = ring_skip(k, w->capacity);
    TG_HIP(launch_window_absorb(e->stream, s->p, w->d, (uint32_t)ring_row(s->drained, skip, ME), (uint32_t)ring_row(w->entered, skip, w->capacity),
                                (int)(k - skip)));
    s->drained += k;
    w->entered += k;
    if (n_absorbed) *n_absorbed = (int32_t)k;
    return TG_OK;
}

int tg_window_push(TgEngine* e, int n, const void* states, const int32_t* n_moves, const TgMove* moves, const uint32_t* visits,
                   const float* results, const int32_t* game_ids) {
    int rc = need_window(e, "tg_window_push");
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!states || !n_moves || !moves || !visits || !results))) return fail(TG_ERR_INVALID_ARG, "tg_window_push: bad arguments");
    Window* w = e->window;
    for (int i = 0; i < n; i++)  // all of them before the first copy: a refused push leaves the window as it was
        if (validate_example(e, i, (const uint8_t*)states, n_moves, visits))
            return fail(TG_ERR_INVALID_ARG, "tg_window_push: example " + std::to_string(i) + " refused, window unchanged: " + tg_last_error());
    if (n == 0) return TG_OK;
    const size_t sb = (size_t)e->g.bytes;
    const uint64_t skip = ring_skip((uint64_t)n, w->capacity);
    const size_t m = (size_t)n - (size_t)skip;
    // canonical rows: nothing past n_moves
    std::vector<TgMove> mv(m * EX_MOVES, 0);
    std::vector<uint32_t> vs(m * EX_MOVES, 0u);
    std::vector<int32_t> ids(m, 0);
    for (size_t i = 0; i < m; i++) {
        const size_t src = (size_t)skip + i, nm = (size_t)n_moves[src];
        std::memcpy(&mv[i * EX_MOVES], moves + src * EX_MOVES, nm * sizeof(TgMove));
        std::memcpy(&vs[i * EX_MOVES], visits + src * EX_MOVES, nm * 4);
        if (game_ids) ids[i] = game_ids[src];
    }
    const uint64_t at = w->entered + skip;
    if ((rc = copy_rows(e, w, w->d.states, (uint8_t*)states + (size_t)skip * sb, sb, at, m, true))) return rc;
    if ((rc = copy_rows(e, w, w->d.n_moves, (void*)(n_moves + skip), 4, at, m, true))) return rc;
    if ((rc = copy_rows(e, w, w->d.result, (void*)(results + skip), 4, at, m, true))) return rc;
    if ((rc = copy_rows(e, w, w->d.game_id, ids.data(), 4, at, m, true))) return rc;
    if ((rc = copy_rows(e, w, w->d.moves, mv.data(), (size_t)EX_MOVES * 2, at, m, true))) return rc;
    if ((rc = copy_rows(e, w, w->d.visits, vs.data(), (size_t)EX_MOVES * 4, at, m, true))) return rc;
    TG_HIP(hipStreamSynchronize(e->stream));  // the staging vectors and the caller's arrays are free again
    w->entered += (uint64_t)n;
    return TG_OK;
}

int tg_window_read(TgEngine* e, int first, int n, TgExampleHeader* headers, void* states, TgMove* moves, uint32_t* visits) {
    int rc = need_window(e, "tg_window_read");
    if (rc) return rc;
    const Window* w = e->window;
    if (first < 0 || n < 0 || (uint64_t)first + (uint64_t)n > w->count())
        return fail(TG_ERR_INVALID_ARG, "tg_window_read: [" + std::to_string(first) + ", " + std::to_string((long long)first + n) +
                                            ") is not inside the window's [0, " + std::to_string(w->count()) + ")");
    if (n > 0 && (!headers || !states || !moves || !visits)) return fail(TG_ERR_INVALID_ARG, "tg_window_read: null argument");
    if (n == 0) return TG_OK;
    const uint64_t at = w->evicted() + (uint64_t)first;
    const size_t m = (size_t)n;
    std::vector<int32_t> nm(m), ids(m);
    std::vector<float> res(m);
    if ((rc = copy_rows(e, w, w->d.states, states, (size_t)e->g.bytes, at, m, false))) return rc;
    if ((rc = copy_rows(e, w, w->d.n_moves, nm.data(), 4, at, m, false))) return rc;
    if ((rc = copy_rows(e, w, w->d.result, res.data(), 4, at, m, false))) return rc;
    if ((rc = copy_rows(e, w, w->d.game_id, ids.data(), 4, at, m, false))) return rc;
    if ((rc = copy_rows(e, w, w->d.moves, moves, (size_t)EX_MOVES * 2, at, m, false))) return rc;
    if ((rc = copy_rows(e, w, w->d.visits, visits, (size_t)EX_MOVES * 4, at, m, false))) return rc;
    TG_HIP(hipStreamSynchronize(e->stream));  // behind an absorb that was still in flight
    for (size_t i = 0; i < m; i++) {
        headers[i].game_id = ids[i];
        headers[i].n_moves = nm[i];
        headers[i].result = res[i];
        headers[i].reserved = 0;
    }
    return TG_OK;
}

int tg_window_train(TgEngine* e, int first, int count, uint64_t seed, float* mean_loss_p, float* mean_loss_z, int32_t* steps) {
    int rc = need_window(e, "tg_window_train");
    if (rc) return rc;
    const Window* w = e->window;
    if (!e->trainer) return fail(TG_ERR_STATE, "tg_window_train: no trainer (tg_train_create)");
    if (first < 0 || count < 0 || (uint64_t)first + (uint64_t)count > w->count())
        return fail(TG_ERR_INVALID_ARG, "tg_window_train: [" + std::to_string(first) + ", " + std::to_string((long long)first + count) +
                                            ") is not inside the window's [0, " + std::to_string(w->count()) + ")");
    return train_window(e, w->d, (uint32_t)ring_row(w->evicted(), (uint64_t)first, w->capacity), count, seed, mean_loss_p, mean_loss_z, steps);
}

}  // extern "C"
