// What the host launch drivers share (dit_launch_dump.cpp, oobleck_launch_dump.cpp; one translation unit each): memory with names, so that
// pointers print as null, alloc<k>+<offset>, ws+<offset> or in:<name>+<offset>; one output line per event; and the HIP runtime calls on host
// memory -- hipMalloc is malloc, recorded in allocation order; copies and memsets are memcpy / memset, so finalize really runs and a host
// sanitizer sees every byte it moves.
#pragma once
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sat_common.h"

// ------------------------------------------------------------------------------ memory with names
namespace {

struct Range {
    const char* base;
    size_t size;
    std::string name;
};
std::vector<Range> g_ranges;          // inputs, workspace and live allocations
int g_allocs = 0;

std::string ptr(const void* p) {
    if (!p) return "null";
    const char* c = (const char*)p;
    const Range* hit = nullptr;
    for (const Range& r : g_ranges)          // one past the end names a range too (an empty carve behind the last one), a range that holds the byte wins
        if (c >= r.base && c <= r.base + r.size && (!hit || c < r.base + r.size)) hit = &r;
    if (!hit) return "unknown";
    const size_t off = (size_t)(c - hit->base);
    return off || hit->name.rfind("in:", 0) != 0 ? hit->name + "+" + std::to_string(off) : hit->name;
}

void put(std::string& o, const void* p) { o += ' ' + ptr(p); }
void put(std::string& o, int v) { o += ' ' + std::to_string(v); }
void put(std::string& o, long v) { o += ' ' + std::to_string(v); }
void put(std::string& o, long long v) { o += ' ' + std::to_string(v); }
void put(std::string& o, size_t v) { o += ' ' + std::to_string(v); }
void put(std::string& o, double v) {
    char b[40];
    snprintf(b, sizeof b, " %.9g", v);
    o += b;
}
void put(std::string& o, const char* label) { o += ' '; o += label; }

template <class... A>
int line(const char* name, A... a) {
    std::string o = name;
    (put(o, a), ...);
    puts(o.c_str());
    return 0;
}

void forget(const void* base) {
    for (size_t i = 0; i < g_ranges.size(); ++i)
        if (g_ranges[i].base == (const char*)base) g_ranges.erase(g_ranges.begin() + i--);
}

// caller-owned buffers: zero-filled, exactly the size the call may touch
struct Inputs {
    std::vector<void*> owned;
    float* make(const std::string& name, size_t floats) {
        void* p = calloc(floats ? floats : 1, 4);
        owned.push_back(p);
        g_ranges.push_back({(const char*)p, floats * 4, "in:" + name});
        return (float*)p;
    }
    void* workspace(size_t bytes) {
        void* p = nullptr;
        if (posix_memalign(&p, 256, bytes ? bytes : 256)) abort();
        owned.push_back(p);
        g_ranges.push_back({(const char*)p, bytes, "ws"});
        return p;
    }
    ~Inputs() {
        for (void* p : owned) {
            forget(p);
            free(p);
        }
    }
};

}  // namespace

// ------------------------------------------------------------------------------ the HIP runtime on host memory
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    *p = malloc(bytes ? bytes : 1);
    g_ranges.push_back({(const char*)*p, bytes, "alloc" + std::to_string(g_allocs++)});
    line("hipMalloc", (const void*)*p, bytes);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    line("hipFree", (const void*)p);
    forget(p);
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    line("hipMemcpyAsync", (const void*)dst, src, bytes, (int)kind);
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t bytes) {
    line("hipMemset", (const void*)dst, v, bytes);
    memset(dst, v, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int v, size_t bytes, hipStream_t) {
    line("hipMemsetAsync", (const void*)dst, v, bytes);
    memset(dst, v, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return line("hipStreamSynchronize"), hipSuccess; }
hipError_t hipDeviceSynchronize() { return line("hipDeviceSynchronize"), hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
}

void sat_set_error(const char* fmt, ...) {
    char b[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    line("error:", (const char*)b);
}

#define RC(fn, ...) line("rc " #fn, (int)fn(__VA_ARGS__))
