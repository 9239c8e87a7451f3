// lcd_runtime.cpp -- the runtime core of liblcd_hotpath.so: the per-thread error string, device selection, the device-memory budget behind DevBuf and the C entry
// points that are about the process and its devices, not about a batch.  Declarations: lcd_host_internal.h.
#include "lcd_host_internal.h"

using namespace lcd_internal;

namespace {

std::mutex g_init_mu;
int g_device = -1;                 // the process default device (lcd_init, else LOCAL_RANK % n, else 0)
thread_local int t_device = -1;    // lcd_set_thread_device: the device of this thread's per-call entry points and of the batches it creates
std::atomic<long long> g_dev_budget[LCD_MAX_DEV];
std::once_flag g_budget_once[LCD_MAX_DEV];
} // namespace

namespace lcd_internal __attribute__((visibility("hidden"))) { // (the attribute does not carry over from the header's block)

thread_local std::string g_err;
int g_n_devices = 0;
int g_n_cus = 256; // compute units of the device (MI355X: 256)
// One process may drive every GPU of the node (the reference's kt_for workers are threads of ONE process, src/call_var_main.c:773): a device belongs
// to an lcd_batch_t (lcd_batch_create_on) or, for the per-call mirrors, to the calling thread (lcd_set_thread_device); nothing is process-global
// except the default.  HIP's current device is per host thread, so every entry point selects its device first.
// GPU_MAX_HW_QUEUES: a submission uses a pool of 4 streams; with more hardware queues holding runnable kernels the queue scheduler time-slices
// them (DESIGN section 4 "Submission").  The host sets GPU_MAX_HW_QUEUES=4 in its environment before its first HIP call; the library
// does not touch the environment of the process it is loaded into.
int init_default_device() {
    std::lock_guard<std::mutex> lk(g_init_mu);
    if (g_device >= 0) return 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return set_err(-1, "liblcd_hotpath: no HIP device visible (this library has no CPU path)"); }
    int dev = 0;
    const char *lr = getenv("LOCAL_RANK");
    if (lr) dev = atoi(lr) % n;
    g_n_devices = n;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) g_n_cus = prop.multiProcessorCount;
    g_device = dev;
    return 0;
}
int use_device(int dev) {
    if (init_default_device()) return -1;
    if (dev < 0) dev = t_device >= 0 ? t_device : g_device;
    if (dev >= g_n_devices) return set_err(-1, "bad device index " + std::to_string(dev));
    if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); return set_err(-1, "hipSetDevice failed"); }
    return 0;
}

// Device memory budget: the library keeps its grow-only buffers under ~92 % of each device (the HIP runtime allocates kernel scratch and
// queue resources lazily at dispatch time -- with HBM full a launch aborts the queue with HSA_STATUS_ERROR_OUT_OF_RESOURCES instead of
// returning an error).  A request over the budget fails like an out-of-memory hipMalloc (-11); lcd_batch_run_many then splits.
std::atomic<long long> g_dev_bytes[LCD_MAX_DEV];
std::atomic<unsigned long long> g_copy_bytes[4]; // [0] digars device -> host, [1] digars host -> device, [2] read bases host -> device (packed or unpacked), [3] read bases device -> host
std::atomic<long long> g_alloc_events{0}; // hipMalloc calls of the grow-only buffers (bench.py reports how many fell into its timed region)
long long dev_budget(int d) {
    std::call_once(g_budget_once[d], [d] {
        size_t fr = 0, tot = 0;
        g_dev_budget[d] = (hipMemGetInfo(&fr, &tot) == hipSuccess && tot > 0) ? (long long)((double)tot * HostSwitches::from_env().mem_fraction) : (1ll << 62);
        (void)hipGetLastError();
    });
    return g_dev_budget[d].load();
}
int DevBuf::ensure(size_t n, int headroom_shift) {
    if (n <= cap) return 0;
    release();
    dev = cur_device();
    const long long budget = dev_budget(dev);
    size_t want = n + (n >> headroom_shift) + 256; // (headroom: the buffers only grow, a slightly larger next batch does not reallocate)
    // the budget is RESERVED before the allocation (compare-exchange): the submission's helper threads grow buffers beside the calling thread
    auto reserve = [&](const size_t bytes) { long long cur = g_dev_bytes[dev].load(); while (cur + (long long)bytes <= budget) if (g_dev_bytes[dev].compare_exchange_weak(cur, cur + (long long)bytes)) return true; return false; };
    if (!reserve(want)) { want = n + 256; if (!reserve(want)) return set_err(-11, "device memory budget: " + std::to_string(want) + " more bytes on top of " + std::to_string(g_dev_bytes[dev].load())); }
    if (hipMalloc(&p, want) != hipSuccess) {
        (void)hipGetLastError(); // out-of-memory is not sticky, but the "last error" slot is read after every launch
        g_dev_bytes[dev] -= (long long)want;
        p = nullptr; cap = 0; return set_err(-11, "hipMalloc failed for " + std::to_string(want) + " bytes");
    }
    if (HostSwitches::from_env().alloc_debug) fprintf(stderr, "[alloc] %zu bytes asked, %zu allocated (device %d now %.2f GB)\n", n, want, dev, g_dev_bytes[dev].load() / 1e9);
    cap = want; ++g_alloc_events; return 0;
}

} // namespace lcd_internal

extern "C" {

int lcd_init(int device) { // the process default device (bench.py: LOCAL_RANK); batches and threads may choose another one
    if (init_default_device()) return -1;
    std::lock_guard<std::mutex> lk(g_init_mu);
    if (device < 0 || device >= g_n_devices) return set_err(-1, "bad device index");
    if (hipSetDevice(device) != hipSuccess) return set_err(-1, "hipSetDevice failed");
    g_device = device;
    return 0;
}
long long lcd_alloc_events(void) { return g_alloc_events.load(); }
void lcd_copy_counters(unsigned long long out[4]) { for (int i = 0; i < 4; ++i) out[i] = g_copy_bytes[i].load(); }
void lcd_account_device_bytes(int device, long long delta) { if (device >= 0 && device < LCD_MAX_DEV) g_dev_bytes[device] += delta; } // (buffers allocated outside DevBuf: lcd_io.cpp's inflated streams)
long long lcd_device_bytes(int device) { return device >= 0 && device < LCD_MAX_DEV ? g_dev_bytes[device].load() : 0; }
int lcd_device_count(void) { return init_default_device() ? 0 : g_n_devices; }
int lcd_set_thread_device(int device) {
    if (init_default_device()) return -1;
    if (device >= g_n_devices) return set_err(-1, "bad device index");
    t_device = device; // < 0: back to the process default
    return use_device(-1);
}
const char *lcd_last_error(void) { return g_err.c_str(); }
const char *lcd_version(void) { return "longcalld_amd hot path 0.1 (gfx950)"; }
int lcd_host_threads(int *team, int *arena_threads, int *cpus, int *local_world) {
    const HostSwitches sw = HostSwitches::from_env();
    if (team) *team = host_team(sw);
    if (arena_threads) *arena_threads = host_arena_threads(sw);
    if (cpus) *cpus = host_cpus();
    if (local_world) *local_world = host_local_world();
    return 0;
}

} // extern "C"
