// Host side of the GEMM: the split-fp16 guard scopes and their thread-local range flag, the deferred range check, and the buffer of the
// diagnostic stamps.  Launches nothing.
#include "common.h"
#include <atomic>

namespace fc {

// the stamp buffer of the diagnostic stamps (knob 20), grown on demand and read back with gemm_read_stamps
static unsigned long long* g_stamp_buf = nullptr;
static size_t g_stamp_cap = 0, g_stamp_n = 0;
unsigned long long* gemm_stamp_buffer(size_t n) {
    if (n > g_stamp_cap) {
        if (g_stamp_buf) FC_HIP(hipFree(g_stamp_buf));
        FC_HIP(hipMalloc(&g_stamp_buf, n * sizeof(unsigned long long)));
        g_stamp_cap = n;
    }
    g_stamp_n = n;
    return g_stamp_buf;
}
size_t gemm_read_stamps(unsigned long long* host, size_t max_n) {
    FC_HIP(hipDeviceSynchronize());
    const size_t n = g_stamp_n < max_n ? g_stamp_n : max_n;
    if (n) FC_HIP(hipMemcpy(host, g_stamp_buf, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return n;
}
static thread_local int* t_fp16_flag = nullptr;
static std::atomic<long> g_fp16_fallbacks{0};

bool gemm_fp16_enabled() { return g_knobs.gemm_variant == 5; }
bool gemm_lnq_ok() { return g_knobs.gemm_variant == 5 && t_fp16_flag != nullptr && g_knobs.lnq_fold; }
bool gemm_limb_chain_all_ok() { return g_knobs.gemm_variant == 5 && t_fp16_flag != nullptr && g_knobs.fused_spline && g_knobs.limb_chain && g_knobs.limb_chain_all; }
bool gemm_limb_chain_ok() { return g_knobs.gemm_variant == 5 && t_fp16_flag != nullptr && g_knobs.fused_spline && g_knobs.limb_chain; }
bool gemm_split_enabled() { return (g_knobs.gemm_variant == 5 || g_knobs.gemm_variant == 3) && g_knobs.fused_spline; }
int* gemm_fp16_flag() { return g_knobs.gemm_variant == 5 ? t_fp16_flag : nullptr; }
int* gemm_scope_flag() { return t_fp16_flag; }
long gemm_fp16_fallbacks() { return g_fp16_fallbacks.load(); }
Fp16Guard::Fp16Guard(int* dev_flag, hipStream_t s) : flag(dev_flag), stream(s), open(true) {
    FC_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
    t_fp16_flag = flag;
}
Fp16Guard::~Fp16Guard() { t_fp16_flag = nullptr; }
Fp16FlagScope::Fp16FlagScope(int* dev_flag) : prev(t_fp16_flag) { t_fp16_flag = dev_flag; }
Fp16FlagScope::~Fp16FlagScope() { t_fp16_flag = prev; }
bool Fp16Guard::overflowed() {
    t_fp16_flag = nullptr;
    open = false;
    int h = 0;
    FC_HIP(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, stream));
    FC_HIP(hipStreamSynchronize(stream));
    if (h) g_fp16_fallbacks.fetch_add(1);
    return h != 0;
}

// ---- deferred range check (common.h).  Per thread: the switch, the queued passes and a pool of pinned flag slots / events.
namespace {
struct DeferredPass { std::function<void()> rerun; int* dev_flag; hipStream_t stream; int* host_flag; hipEvent_t ev; int device; };
struct DeferState {
    bool on = false;
    std::vector<DeferredPass> pending;
    struct Slot { int* host_flag; hipEvent_t ev; int device; };      // (an event belongs to the device that was current when it was created)
    std::vector<Slot> pool;
    ~DeferState() {
        for (auto& pe : pool) { (void)hipHostFree(pe.host_flag); (void)hipEventDestroy(pe.ev); }
        for (auto& d : pending) { (void)hipHostFree(d.host_flag); (void)hipEventDestroy(d.ev); }
    }
};
thread_local DeferState t_defer;
}  // namespace
bool guard_deferred() { return t_defer.on; }
int guard_pending() { return (int)t_defer.pending.size(); }
void guard_set_deferred(bool on) { t_defer.on = on; }
void Fp16Guard::defer(std::function<void()> rerun) {
    t_fp16_flag = nullptr;
    open = false;
    DeferredPass d{std::move(rerun), flag, stream, nullptr, nullptr, 0};
    FC_HIP(hipGetDevice(&d.device));                 // the pass may be repeated from a call made with another device current
    for (size_t i = t_defer.pool.size(); i-- > 0;)
        if (t_defer.pool[i].device == d.device) {
            d.host_flag = t_defer.pool[i].host_flag; d.ev = t_defer.pool[i].ev;
            t_defer.pool.erase(t_defer.pool.begin() + (long)i);
            break;
        }
    if (!d.host_flag) {
        FC_HIP(hipHostMalloc((void**)&d.host_flag, sizeof(int), hipHostMallocDefault));
        FC_HIP(hipEventCreateWithFlags(&d.ev, hipEventDisableTiming));
    }
    *d.host_flag = 0;
    FC_HIP(hipMemcpyAsync(d.host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, stream));
    FC_HIP(hipEventRecord(d.ev, stream));
    t_defer.pending.push_back(std::move(d));
}
int guard_resolve() {
    int repeated = 0;
    std::vector<DeferredPass> todo;
    todo.swap(t_defer.pending);
    std::exception_ptr err;
    int dev_entry = 0;
    (void)hipGetDevice(&dev_entry);
    for (DeferredPass& d : todo) {
        try {
            if (err) (void)hipEventSynchronize(d.ev);        // error path: the flag copy behind this event still targets d.host_flag -- wait before the slot is pooled
            if (!err) {
                FC_HIP(hipSetDevice(d.device));              // re-launches go to the device (and pointers) the pass was queued on
                FC_HIP(hipEventSynchronize(d.ev));
                if (*d.host_flag) {                          // the fast pass left fp16's range: the whole pass again on the bf16-limb loops
                    g_fp16_fallbacks.fetch_add(1);
                    d.rerun();
                    ++repeated;
                } else if (repeated) {                       // an earlier pass was repeated and may feed this one: fast pass again, checked at once
                    bool over;
                    { Fp16Guard g(d.dev_flag, d.stream); d.rerun(); over = g.overflowed(); }
                    if (over) d.rerun();
                    ++repeated;
                }
            }
        } catch (...) { err = std::current_exception(); }
        t_defer.pool.push_back({d.host_flag, d.ev, d.device});
    }
    (void)hipSetDevice(dev_entry);
    if (err) std::rethrow_exception(err);
    return repeated;
}

}  // namespace fc
