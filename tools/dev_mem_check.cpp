// dev_mem_check.cpp — a stand-alone host run of the ownership helpers of qdrant_amd/csrc/dev_mem.hpp (DevBuf, Staging, dev_upload) against a fake
// HIP allocator: hipMalloc / hipFree / hipMemcpy backed by malloc, a set of live pointers, and a call counter that makes the k-th allocation or copy
// fail.  Functions written the way the one-shot entry points of api_*.hip are written run once clean and once per failing call; after every run
// nothing may be live, nothing freed twice, and the failure's code must come back.  No GPU, no HIP runtime.  Meant for the sanitizers:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iqdrant_amd/csrc
//       tools/dev_mem_check.cpp -o /tmp/dev_mem_check      (one command line)
//   /tmp/dev_mem_check
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "dev_mem.hpp"

using namespace qmx;

// ---- the fake runtime ----
namespace {
std::set<void *> live;            // "device" allocations
int calls = 0;                    // allocations + copies so far
int fail_at = 0;                  // the call that fails (1-based; 0 = none)
int bad_frees = 0;                // hipFree of something not live (a double free included)
int copies = 0;
std::string last_error;

bool failing() { return ++calls == fail_at; }
void reset(int k) {
    calls = 0;
    copies = 0;
    fail_at = k;
    last_error.clear();
}
}  // namespace

extern "C" hipError_t hipMalloc(void **ptr, size_t size) {
    if (failing()) {
        *ptr = nullptr;
        return hipErrorOutOfMemory;
    }
    *ptr = malloc(size ? size : 1);
    live.insert(*ptr);
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *ptr) {
    if (!live.erase(ptr)) {
        ++bad_frees;
        return hipErrorInvalidValue;
    }
    free(ptr);
    return hipSuccess;
}
extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) {
    if (failing()) return hipErrorInvalidValue;
    ++copies;
    memcpy(dst, src, bytes);
    return hipSuccess;
}

namespace qmx {
void set_error(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error = buf;
}
int32_t hip_status(hipError_t e, const char *what, const char *, int) {
    set_error("%s: HIP error %d", what, (int)e);
    return e == hipErrorOutOfMemory ? QMX_ERR_OUT_OF_MEMORY : QMX_ERR_OTHER;
}
bool is_device_ptr(const void *p) { return live.count(const_cast<void *>(p)) != 0; }
}  // namespace qmx

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

namespace {

// ---- functions in the shape of the rewritten entry points ----
int32_t launch_double(const float *d_in, size_t n, float *d_out) {      // (the "kernel": device memory is host memory here)
    for (size_t i = 0; i < n; ++i) d_out[i] = 2.0f * d_in[i];
    return QMX_OK;
}

// qmx_cast_f32 / qmx_preprocess_f32: one input, one output.  Written with two hand-released buffers this leaked the first when the second failed.
int32_t encode_like(const float *in, size_t n, float *out) {
    Staging st;
    const float *d_in = nullptr;
    float *d_out = nullptr;
    QMX_TRY(st.in(in, n * 4, &d_in));
    QMX_TRY(st.out(out, n * 4, &d_out));
    QMX_TRY(launch_double(d_in, n, d_out));
    return st.back();
}

// qmx_merge_topk / qmx_pq_encode: two inputs, two outputs, a scratch buffer and a launch
int32_t two_in_two_out(const float *a, const float *b, size_t n, float *sum, float *diff) {
    Staging st;
    DevBuf scratch;
    const float *d_a = nullptr, *d_b = nullptr;
    float *d_sum = nullptr, *d_diff = nullptr;
    QMX_TRY(st.in(a, n * 4, &d_a));
    QMX_TRY(st.in(b, n * 4, &d_b));
    QMX_TRY(st.out(sum, n * 4, &d_sum));
    QMX_TRY(st.out(diff, n * 4, &d_diff));
    QMX_TRY(scratch.reserve(n * 4));
    float *t = (float *)scratch.p;
    for (size_t i = 0; i < n; ++i) {
        t[i] = d_b[i];
        d_sum[i] = d_a[i] + t[i];
        d_diff[i] = d_a[i] - t[i];
    }
    return st.back();
}

// a handle whose destructor frees its fields, and a create function that deletes the half-built handle
struct Handle {
    float *d_x = nullptr;
    uint32_t *d_y = nullptr;
    DevBuf extra;
    ~Handle() {
        dev_free(d_x);
        dev_free(d_y);
    }
};
int32_t handle_fill(Handle *h, const float *x, const uint32_t *y, size_t n) {
    QMX_TRY(dev_upload(&h->d_x, x, n));
    QMX_TRY(dev_upload(&h->d_y, y, n));
    QMX_TRY(dev_upload(h->extra, y, n));
    return QMX_OK;
}
int32_t handle_create(const float *x, const uint32_t *y, size_t n, Handle **out) {
    *out = nullptr;
    Handle *h = new Handle();
    const int32_t rc = handle_fill(h, x, y, n);
    if (rc != QMX_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return QMX_OK;
}

// runs `f` clean, then once per call of the clean run with that call failing
template <class F> int sweep(const char *name, F f) {
    reset(0);
    CHECK(f() == QMX_OK);
    const int n_calls = calls;
    CHECK(n_calls > 0 && live.empty() && bad_frees == 0);
    for (int k = 1; k <= n_calls; ++k) {
        reset(k);
        const int32_t rc = f();
        const bool was_alloc = last_error.find("hipMalloc") != std::string::npos;
        CHECK(rc == (was_alloc ? QMX_ERR_OUT_OF_MEMORY : QMX_ERR_OTHER));
        CHECK(!last_error.empty());
        CHECK(live.empty());
        CHECK(bad_frees == 0);
    }
    printf("%-16s %2d calls, every one failed once: nothing live, nothing freed twice\n", name, n_calls);
    return n_calls;
}

void check_devbuf() {
    reset(0);
    {
        DevBuf b;
        CHECK(b.reserve(10) == QMX_OK && b.cap == 4096 && live.size() == 1);      // the floor
        void *first = b.p;
        CHECK(b.reserve(100) == QMX_OK && b.p == first && calls == 1);            // fits: no new allocation
        CHECK(b.reserve(5000) == QMX_OK && b.cap == 5000 && live.size() == 1 && calls == 2);      // growth frees, then allocates
        DevBuf c(std::move(b));                                                   // move construction
        CHECK(b.p == nullptr && b.cap == 0 && c.cap == 5000 && live.size() == 1);
        DevBuf d;
        CHECK(d.reserve(64) == QMX_OK && live.size() == 2);
        d = std::move(c);                                                         // move assignment frees what d held
        CHECK(c.p == nullptr && d.cap == 5000 && live.size() == 1);
        DevBuf &self = d;
        d = std::move(self);                                                      // self-assignment keeps it
        CHECK(d.cap == 5000 && live.size() == 1);
        void *raw = d.detach();                                                   // detach hands the allocation over
        CHECK(d.p == nullptr && d.cap == 0 && live.count(raw) == 1);
        (void)hipFree(raw);
        // a failed growth leaves an empty buffer, not a dangling one
        DevBuf e;
        CHECK(e.reserve(16) == QMX_OK);
        fail_at = calls + 1;
        CHECK(e.reserve(1 << 20) == QMX_ERR_OUT_OF_MEMORY && e.p == nullptr && e.cap == 0);
    }
    CHECK(live.empty() && bad_frees == 0);
    printf("DevBuf           floor, growth, moves, detach, failed growth\n");
}

void check_staging() {
    const size_t n = 37;
    std::vector<float> in(n), out(n, -1.0f), untouched(n, -1.0f);
    for (size_t i = 0; i < n; ++i) in[i] = (float)i;
    // host -> host
    reset(0);
    CHECK(encode_like(in.data(), n, out.data()) == QMX_OK);
    for (size_t i = 0; i < n; ++i) CHECK(out[i] == 2.0f * (float)i);
    CHECK(calls == 4 && copies == 2 && live.empty());      // two allocations, one copy in, one copy back
    // device -> device: nothing staged, nothing copied
    float *d_in = nullptr, *d_out = nullptr;
    CHECK(dev_upload(&d_in, in.data(), n) == QMX_OK && dev_upload(&d_out, untouched.data(), n) == QMX_OK);
    reset(0);
    CHECK(encode_like(d_in, n, d_out) == QMX_OK && calls == 0 && live.size() == 2);
    for (size_t i = 0; i < n; ++i) CHECK(d_out[i] == 2.0f * (float)i);
    // back() copies the staged outputs only, once: a device output, a null output and an empty one are left alone
    {
        Staging st;
        float *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
        reset(0);
        CHECK(st.out(out.data(), n * 4, &a) == QMX_OK && a != out.data() && is_device_ptr(a));
        CHECK(st.out(d_out, n * 4, &b) == QMX_OK && b == d_out);
        CHECK(st.out((float *)nullptr, n * 4, &c) == QMX_OK && c == nullptr);
        CHECK(st.out(untouched.data(), 0, &d) == QMX_OK && d == untouched.data());
        CHECK(calls == 1);
        for (size_t i = 0; i < n; ++i) a[i] = 7.0f;
        CHECK(st.back() == QMX_OK && copies == 1);
        CHECK(st.back() == QMX_OK && copies == 1);
        for (size_t i = 0; i < n; ++i) CHECK(out[i] == 7.0f && untouched[i] == -1.0f);
        // inout: the host content goes in, the device's result comes back
        float *e = nullptr;
        CHECK(st.inout(out.data(), n * 4, &e) == QMX_OK && e != out.data() && e[3] == 7.0f);
        e[3] = 9.0f;
        CHECK(st.back() == QMX_OK && out[3] == 9.0f);
    }
    dev_free(d_in);
    dev_free(d_out);
    CHECK(d_in == nullptr && live.empty() && bad_frees == 0);
    printf("Staging          four placements, back() copies staged outputs only\n");
}

}  // namespace

int main() {
    check_devbuf();
    check_staging();
    const size_t n = 37;
    std::vector<float> a(n, 3.0f), b(n, 1.0f), s(n), d(n);
    std::vector<uint32_t> y(n, 5u);
    // the leak of the hand-released shape: the second allocation fails after the first succeeded
    reset(3);      // calls: hipMalloc(in), hipMemcpy(in), hipMalloc(out)
    CHECK(encode_like(a.data(), n, s.data()) == QMX_ERR_OUT_OF_MEMORY && live.empty() && bad_frees == 0);
    printf("encode_like      second allocation fails after the first succeeded: nothing live\n");
    sweep("encode_like", [&] { return encode_like(a.data(), n, s.data()); });
    const int c2 = sweep("two_in_two_out", [&] { return two_in_two_out(a.data(), b.data(), n, s.data(), d.data()); });
    CHECK(c2 == 4 + 2 + 1 + 2);      // four staging allocations, two copies in, the scratch, two copies back
    for (size_t i = 0; i < n; ++i) CHECK(s[i] == 4.0f && d[i] == 2.0f);      // (the clean run's result; a failed run writes no host output early)
    sweep("handle_create", [&] {
        Handle *h = nullptr;
        const int32_t rc = handle_create(a.data(), y.data(), n, &h);
        CHECK((rc == QMX_OK) == (h != nullptr));
        if (h) {
            CHECK(live.size() == 3 && h->d_y[n - 1] == 5u);
            delete h;
        }
        return rc;
    });
    // zero elements still allocate one (the handles' fields are never null after a create)
    reset(0);
    uint32_t *z = nullptr;
    CHECK(dev_upload(&z, (const uint32_t *)nullptr, 0) == QMX_OK && z && copies == 0);
    dev_free(z);
    CHECK(live.empty() && bad_frees == 0);
    printf("ok\n");
    return 0;
}
