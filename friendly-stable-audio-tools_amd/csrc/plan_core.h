// The host-side lifecycle every plan shares (dit_plan.hip, oobleck_plan.hip, t5_encoder.hip, roberta_encoder.hip):
// create -> set_tensor (name -> caller's fp32 device pointer) -> finalize (count the arena, allocate it, copy / re-pack into it,
// synchronise, forget the pointers) -> per-call workspace carved with the same allocator -> destroy.  Host code only, internal linkage.
#pragma once
#include <map>
#include <string>

#include "sat_common.h"

namespace {

// Bump allocator over an optional base in 256-byte steps; with a null base it only counts (the first pass of finalize, *_workspace_bytes)
struct Bump {
    char* base = nullptr;
    size_t off = 0;
    bool dry() const { return !base; }
    size_t take_off(size_t bytes) {
        const size_t o = off;
        off += (size_t)round_up((int64_t)bytes, 256);
        return o;
    }
    void* take(size_t bytes) {
        const size_t o = take_off(bytes);
        return base ? base + o : nullptr;
    }
};

// Owning device buffer: grows on request, never shrinks, freed with the plan
struct DevBuf {
    char* ptr = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
    // reallocates (contents lost) only when `bytes` exceeds the capacity; work queued on the old buffer is the caller's to wait for
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        SAT_HIP(hipMalloc((void**)&ptr, bytes));
        cap = bytes;
        return 0;
    }
};

// name -> (caller's device pointer, elements) between set_tensor and finalize; `what` is the plan kind in the messages ("dit", "t5", ...)
struct TensorTable {
    std::map<std::string, std::pair<const float*, int64_t>> m;
    int set(const char* what, const char* name, const float* data_dev, int64_t numel) {
        SAT_CHECK_ARG(name && data_dev && numel > 0, SAT_E_INVALID, "%s_plan_set_tensor: bad argument", what);
        m[name] = {data_dev, numel};
        return 0;
    }
    bool has(const std::string& name) const { return m.count(name) != 0; }
    int64_t numel(const std::string& name) const {          // 0: never set
        auto it = m.find(name);
        return it == m.end() ? 0 : it->second.second;
    }
    // first_rows: the first `numel` elements of a table of whole rows of `numel` (RoBERTa's token-type table)
    int get(const char* what, const std::string& name, int64_t numel, const float** out, bool first_rows = false) const {
        auto it = m.find(name);
        SAT_CHECK_ARG(it != m.end(), SAT_E_MISSING, "%s plan: tensor '%s' was never set", what, name.c_str());
        const int64_t have = it->second.second;
        SAT_CHECK_ARG(first_rows ? (have >= numel && have % numel == 0) : have == numel, SAT_E_INVALID,
                      "%s plan: tensor '%s' has %lld elements, expected %lld", what, name.c_str(), (long long)have, (long long)numel);
        *out = it->second.first;
        return 0;
    }
    // the named tensor, checked, copied to dst (device to device)
    int copy(const char* what, const std::string& name, int64_t numel, float* dst, hipStream_t s, bool first_rows = false) const {
        const float* src;
        SAT_TRY(get(what, name, numel, &src, first_rows));
        SAT_HIP(hipMemcpyAsync(dst, src, (size_t)numel * 4, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    // finalize, both passes: the named tensor takes the arena's next `numel` floats; copied there unless the pass only counts
    int place(const char* what, Bump& ar, const std::string& name, int64_t numel, float** dst, hipStream_t s, bool first_rows = false) const {
        *dst = (float*)ar.take((size_t)numel * 4);
        return ar.dry() ? 0 : copy(what, name, numel, *dst, s, first_rows);
    }
    void clear() { m.clear(); }
};

// finalize of a plan with members `tensors`, `arena`, `finalized`: build(Bump&) runs twice, counting and then copying.  The stream is
// synchronised before returning, so the caller may free its fp32 tensors.  On failure the plan stays unfinalized and keeps its table:
// the caller may set what was missing and finalize again, or destroy the plan.
template <class Plan, class Build>
int plan_finalize(Plan* p, hipStream_t s, Build build) {
    p->finalized = false;
    Bump count;
    SAT_TRY(build(count));
    p->arena.release();
    SAT_TRY(p->arena.reserve(count.off));
    Bump place{p->arena.ptr};
    SAT_TRY(build(place));
    SAT_HIP(hipStreamSynchronize(s));
    p->tensors.clear();
    p->finalized = true;
    return 0;
}

}  // namespace
