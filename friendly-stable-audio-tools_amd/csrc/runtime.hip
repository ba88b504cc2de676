// Runtime plumbing of the library: the thread-local error text behind sat_last_error, the per-kernel dynamic-LDS opt-in, the
// compute-unit count of the current device, the ABI version.  Host code only; no kernel.
#include <stdarg.h>

#include <atomic>
#include <mutex>
#include <set>
#include <string>

#include "sat_common.h"

// ------------------------------------------------------------------------------ errors
static thread_local std::string g_last_error;
void sat_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}
extern "C" const char* sat_last_error(void) { return g_last_error.c_str(); }

int sat_ensure_dynamic_lds(const void* kernel, int bytes) {
    // Launch-path cost: one thread-local table probe (no lock, no allocation) once a (kernel, device) pair has been seen by this
    // thread; the mutex-protected set is only consulted on a thread's first launch of a kernel on a device.
    struct Seen { const void* k; int dev; };
    static thread_local Seen seen[64];
    static thread_local int n_seen = 0;
    int dev = 0;
    SAT_HIP(hipGetDevice(&dev));
    for (int i = 0; i < n_seen; ++i)
        if (seen[i].k == kernel && seen[i].dev == dev) return 0;
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (!done.count({kernel, dev})) {
            SAT_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
            done.insert({kernel, dev});
        }
    }
    if (n_seen < 64) seen[n_seen++] = Seen{kernel, dev};
    return 0;
}
// compute units of the current device: one attribute query per device and process (no allocation, no synchronisation); 0 on failure
int sat_device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        sat_set_error("hipGetDevice failed");
        return 0;
    }
    int c = (dev >= 0 && dev < 64) ? cache[dev].load(std::memory_order_relaxed) : 0;
    if (!c) {
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) {
            sat_set_error("hipDeviceGetAttribute(MultiprocessorCount) failed");
            return 0;
        }
        if (dev >= 0 && dev < 64) cache[dev].store(c, std::memory_order_relaxed);
    }
    return c;
}
extern "C" int sat_version(void) { return 6; }
