// C-ABI of dsptoolbox_amd (see include/dsptoolbox_amd.h): context, memory,
// plan (twiddle) cache, launch logic.  gfx950 only.
#include <dlfcn.h>
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dsptoolbox_amd.h"
#include "config.hpp"
#include "host_marshal.hpp"
#include "carry_tables.hpp"
#include "kernels_bigfft.hpp"
#include "kernels_bluestein.hpp"
#include "kernels_finish.hpp"
#include "kernels_csm_b3.hpp"
#include "kernels_generic.hpp"
#include "kernels_welch4096.hpp"
#include "kernels_welch4096w.hpp"
#include "kernels_fir16k.hpp"
#include "kernels_fir4k.hpp"
#include "kernels_stft4096.hpp"
#include "kernels_deconv8k.hpp"
#include "kernels_stft1024.hpp"
#include "kernels_welch1024.hpp"
#include "kernels_welch8192.hpp"
#include "kernels_welch16384.hpp"
#include "kernels_welch_long.hpp"
#include "kernels_stft_long.hpp"
#include "kernels_welch2048h.hpp"
#include "kernels_istft_long.hpp"
#include "kernels_welch_f64.hpp"
#include "kernels_stft_any.hpp"
#include "kernels_fir_stream.hpp"
#include "kernels_freqz.hpp"
#include "kernels_beamform.hpp"
#include "kernels_iir.hpp"
#include "kernels_ciir.hpp"
#include "kernels_dist.hpp"
#include "kernels_delay.hpp"
#include "kernels_cwt.hpp"
#include "kernels_smooth.hpp"
#include "kernels_direct.hpp"
#include "kernels_fft64.hpp"
#include "kernels_latency.hpp"
#include "kernels_lpc.hpp"
#include "kernels_warp.hpp"
#include "kernels_sfilt.hpp"
#include "kernels_rtfilt.hpp"
#include "kernels_room.hpp"
#include "kernels_vqt.hpp"
#include "kernels_fx.hpp"
#include "kernels_specsub.hpp"
#include "kernels_level.hpp"
#include "kernels_resample.hpp"
#include "size_guards.hpp"

using namespace dsk;

static thread_local std::string g_err;

struct ds_ctx {
    int device = 0;
    ds_config cfg;  // every DSPTOOLBOX_AMD_* switch, read once by ds_init (config.hpp)
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;  // second stream for a kernel that may run beside the main one
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_chunk[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // csm_chunked_run
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    std::map<int, float2*> tw;  // twiddle tables by length
    // Bluestein chirp-filter spectra by (L, M): a least-recently-used cache under a byte cap (a
    // table is M float2, up to 128 MB; recordings of ever-changing lengths must not pin one each)
    struct BlueEntry {
        float2* ptr;
        size_t bytes;
        uint64_t stamp;
    };
    std::map<std::pair<int64_t, int64_t>, BlueEntry> blue;
    size_t blue_bytes = 0;
    uint64_t blue_clock = 0;
    // float64 transforms (kernels_fft64.hpp): the 8192-point twiddle table, and per length n Bluestein's chirp w [n]
    // followed by the spectrum of its filter [M] in one allocation, least recently used out under a byte cap
    double2* fft64_tw = nullptr;
    struct Blue64Entry {
        double2* ptr;
        size_t bytes;
        uint64_t stamp;
    };
    std::map<int64_t, Blue64Entry> blue64;
    size_t blue64_bytes = 0;
    float2* w4_tables = nullptr;  // welch4096::host_tables()
    float2* stft_dif_tw[2] = {nullptr, nullptr};  // stft4k::host_twiddles(8192 / 16384)
    float2* fir16k_tables = nullptr;  // fir16k::host_tables()
    float2* wl_tables[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // welchl::host_tables(R), R = 2, 4, ..., 64
    float2* deconv8k_tables = nullptr;  // deconv8k::host_tables()
    float2* deconv_rperm = nullptr;     // deconv8k::k_rperm's output (64 KB), rewritten by every ds_deconv_dev call that uses it
    int n_cu = 0;                       // compute units of the device (persistent grids)
    float2* stft1k_tables = nullptr;  // stft1k::host_tables<1024>()
    float2* stft_wave_tables[3] = {nullptr, nullptr, nullptr};  // stft1k::host_tables<512>(), <256>(), <2048>()
    void* ws = nullptr;         // kernel workspace (spectra, partials)
    size_t ws_bytes = 0;
    void* io = nullptr;  // staging for the host-pointer entry points
    size_t io_bytes = 0;
    void* aux = nullptr;  // small persistent scratch (combined FIR taps, cascade ping-pong buffer)
    void* frames = nullptr;  // time-domain frames of the inverse STFT with a non-power-of-two length
    size_t frames_bytes = 0;
    void* pin[2] = {nullptr, nullptr};  // pinned host chunks of the fused float64 upload (double buffer)
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_busy[2] = {false, false};
    size_t aux_bytes = 0;
    // RCCL (dlopen'ed lazily)
    void* rccl = nullptr;
    void* comm = nullptr;
    // per-kernel HIP-event timing (ds_profile_*)
    bool prof = false;
    struct ProfRec {
        const char* name;
        hipEvent_t a, b;
    };
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    std::string prof_text;
    std::string prof_only;  // non-empty: only launches of this kernel name are bracketed
    int prof_stride = 1;    // bracket every prof_stride-th matching launch (an event pair costs ~3 us of stream time)
    long prof_seen = 0;
    std::set<const char*> routes;                     // launch names ("group@variant" literals) since the last ds_routes()
    std::map<const char*, std::string> group_names;   // "group@variant" literal -> "group"
    std::string routes_text;
};

static int fail(ds_ctx* c, int code, const std::string& msg) {
    g_err = msg;
    if (c) c->err = msg;
    return code;
}
// "<who>: <what>": how an entry that shares its checks with a twin names itself in the message
static int fail(ds_ctx* c, int code, const char* who, const char* what) {
    return fail(c, code, std::string(who) + ": " + what);
}
#define HIPCHK(c, expr)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(c, DS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define CHK(expr)                 \
    do {                          \
        int r_ = (expr);          \
        if (r_ != DS_OK) return r_; \
    } while (0)

static bool is_pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }
static bool fb_mode_ok(int mode) { return mode == DS_FB_PARALLEL || mode == DS_FB_SUMMED || mode == DS_FB_SEQUENTIAL; }
static const int kMaxFft = 16384, kMinFft = 8;
static const int64_t kMaxBigFft = (int64_t)1 << 24;  // four-step path (kernels_bigfft.hpp)

extern "C" int ds_version(void) { return 100; }

// ---- host marshalling helpers (no device work): csrc/host_marshal.hpp --------
using dshost::host_parallel;
using dshost::host_threads;
extern "C" int ds_host_planar_f32(const double* src, int64_t n_samples, int n_ch, float* dst, int64_t ld,
                                  int threads) {
    if (!src || !dst || n_samples < 0 || n_ch <= 0 || ld < n_samples)
        return fail(nullptr, DS_ERR_ARG, "ds_host_planar_f32: bad argument");
    dshost::planar_f32(src, n_samples, n_ch, dst, ld, host_threads(threads, n_samples * n_ch));
    return DS_OK;
}
extern "C" int ds_host_widen_f64(const float* src, int64_t n, double* dst, int threads) {
    if (!src || !dst || n < 0) return fail(nullptr, DS_ERR_ARG, "ds_host_widen_f64: bad argument");
    dshost::widen_f64(src, n, dst, host_threads(threads, n));
    return DS_OK;
}
extern "C" int ds_host_interleave_f64(const float* src, int64_t n_samples, int n_ch, int64_t ld, double* dst,
                                      int threads) {
    if (!src || !dst || n_samples < 0 || n_ch <= 0 || ld < n_samples)
        return fail(nullptr, DS_ERR_ARG, "ds_host_interleave_f64: bad argument");
    dshost::interleave_f64(src, n_samples, n_ch, ld, dst, host_threads(threads, n_samples * n_ch));
    return DS_OK;
}
extern "C" int ds_max_fft_len(void) { return kMaxFft; }
extern "C" int ds_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int ds_init(int device, ds_ctx** out) {
    if (!out) return fail(nullptr, DS_ERR_ARG, "ds_init: out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(nullptr, DS_ERR_HIP, "ds_init: no HIP device visible");
    if (device < 0 || device >= n) return fail(nullptr, DS_ERR_ARG, "ds_init: bad device index");
    ds_ctx* c = new ds_ctx();
    c->device = device;
    c->cfg = ds_config::from_env();
    HIPCHK(c, hipSetDevice(device));
    HIPCHK(c, hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device));
    HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    HIPCHK(c, hipEventCreate(&c->ev0));
    HIPCHK(c, hipEventCreate(&c->ev1));
    *out = c;
    return DS_OK;
}

extern "C" int ds_comm_destroy(ds_ctx* c);

extern "C" void ds_destroy(ds_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    ds_comm_destroy(c);
    (void)hipStreamSynchronize(c->stream);
    for (auto& kv : c->tw) (void)hipFree(kv.second);
    if (c->w4_tables) (void)hipFree(c->w4_tables);
    for (float2* t : c->stft_dif_tw)
        if (t) (void)hipFree(t);
    if (c->fir16k_tables) (void)hipFree(c->fir16k_tables);
    for (auto t : c->wl_tables)
        if (t) (void)hipFree(t);
    if (c->deconv8k_tables) (void)hipFree(c->deconv8k_tables);
    if (c->deconv_rperm) (void)hipFree(c->deconv_rperm);
    if (c->stft1k_tables) (void)hipFree(c->stft1k_tables);
    for (float2* t : c->stft_wave_tables)
        if (t) (void)hipFree(t);
    for (auto& kv : c->blue) (void)hipFree(kv.second.ptr);
    for (auto& kv : c->blue64) (void)hipFree(kv.second.ptr);
    if (c->fft64_tw) (void)hipFree(c->fft64_tw);
    for (auto& r : c->prof_recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto& e : c->prof_pool) (void)hipEventDestroy(e);
    if (c->ws) (void)hipFree(c->ws);
    if (c->io) (void)hipFree(c->io);
    if (c->aux) (void)hipFree(c->aux);
    if (c->frames) (void)hipFree(c->frames);
    for (int i = 0; i < 2; ++i) {
        if (c->pin[i]) (void)hipHostFree(c->pin[i]);
        if (c->pin_ev[i]) (void)hipEventDestroy(c->pin_ev[i]);
    }
    (void)hipEventDestroy(c->ev0);
    (void)hipEventDestroy(c->ev1);
    (void)hipStreamDestroy(c->stream);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (auto e : c->ev_chunk)
        if (e) (void)hipEventDestroy(e);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    delete c;
}

extern "C" const char* ds_last_error(ds_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }

extern "C" int ds_malloc(ds_ctx* c, void** dptr, size_t bytes) {
    if (!c || !dptr) return fail(c, DS_ERR_ARG, "ds_malloc: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(c, DS_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return DS_OK;
}
extern "C" int ds_free(ds_ctx* c, void* dptr) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_free: null ctx");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(dptr));
    return DS_OK;
}
extern "C" int ds_host_alloc(ds_ctx* c, void** hptr, size_t bytes) {
    if (!c || !hptr) return fail(c, DS_ERR_ARG, "ds_host_alloc: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, DS_ERR_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return DS_OK;
}
extern "C" int ds_host_free(ds_ctx* c, void* hptr) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_host_free: null ctx");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipHostFree(hptr));
    return DS_OK;
}
extern "C" int ds_upload(ds_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return fail(c, DS_ERR_ARG, "ds_upload: null argument");
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DS_OK;
}
extern "C" int ds_download(ds_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return fail(c, DS_ERR_ARG, "ds_download: null argument");
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DS_OK;
}
extern "C" int ds_memset(ds_ctx* c, void* dst, int value, size_t bytes) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_memset: null ctx");
    HIPCHK(c, hipMemsetAsync(dst, value, bytes, c->stream));
    return DS_OK;
}
extern "C" int ds_sync(ds_ctx* c) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_sync: null ctx");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DS_OK;
}
extern "C" int ds_timer_start(ds_ctx* c) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_timer_start: null ctx");
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    return DS_OK;
}
extern "C" int ds_timer_stop(ds_ctx* c, float* ms) {
    if (!c || !ms) return fail(c, DS_ERR_ARG, "ds_timer_stop: null argument");
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return DS_OK;
}

extern "C" int ds_profile_enable(ds_ctx* c, int on) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_profile_enable: null ctx");
    c->prof = on != 0;
    return DS_OK;
}

extern "C" int ds_profile_only(ds_ctx* c, const char* kernel_name) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_profile_only: null ctx");
    c->prof_only = kernel_name ? kernel_name : "";
    return DS_OK;
}

extern "C" int ds_profile_stride(ds_ctx* c, int every) {
    if (!c || every < 1) return fail(c, DS_ERR_ARG, "ds_profile_stride: bad argument");
    c->prof_stride = every;
    c->prof_seen = 0;
    return DS_OK;
}

// What an event pair adds to the kernels it brackets: `n_kernels` empty kernels bracketed exactly as
// launch() does it, behind another kernel on the same stream (the start event then waits for a
// predecessor, as in a real step).  Average elapsed time over `reps` brackets, in ms.  With
// b1 = one and b2 = two kernels inside, b2 - b1 is what an empty kernel costs in the stream and
// 2 b1 - b2 a lower bound of the bracket's fixed cost.
__global__ void k_profile_nop() {}
static int prof_event(ds_ctx* c, hipEvent_t* ev);
extern "C" int ds_profile_overhead(ds_ctx* c, int reps, int n_kernels, double* ms) {
    if (!c || !ms || reps < 1 || n_kernels < 1) return fail(c, DS_ERR_ARG, "ds_profile_overhead: bad argument");
    hipEvent_t a, b;
    CHK(prof_event(c, &a));
    CHK(prof_event(c, &b));
    double sum = 0.0;
    for (int i = 0; i < reps; ++i) {
        hipLaunchKernelGGL(k_profile_nop, dim3(1), dim3(64), 0, c->stream);
        HIPCHK(c, hipEventRecord(a, c->stream));
        for (int k = 0; k < n_kernels; ++k) hipLaunchKernelGGL(k_profile_nop, dim3(1), dim3(64), 0, c->stream);
        HIPCHK(c, hipEventRecord(b, c->stream));
        HIPCHK(c, hipEventSynchronize(b));
        float e = 0.f;
        HIPCHK(c, hipEventElapsedTime(&e, a, b));
        sum += e;
    }
    c->prof_pool.push_back(a);
    c->prof_pool.push_back(b);
    *ms = sum / reps;
    return DS_OK;
}

// "name total_ms count\n" per kernel since the last call; synchronises the stream
extern "C" const char* ds_profile_report(ds_ctx* c) {
    if (!c) return "";
    (void)hipStreamSynchronize(c->stream);
    std::map<std::string, std::pair<double, long>> acc;
    for (auto& r : c->prof_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            auto& e = acc[r.name];
            e.first += ms;
            e.second += 1;
        }
        c->prof_pool.push_back(r.a);
        c->prof_pool.push_back(r.b);
    }
    c->prof_recs.clear();
    c->prof_text.clear();
    char line[256];
    for (auto& kv : acc) {
        snprintf(line, sizeof line, "%s %.6f %ld\n", kv.first.c_str(), kv.second.first, kv.second.second);
        c->prof_text += line;
    }
    return c->prof_text.c_str();
}

// launch names since the last call, space separated, each "group" or "group@variant" (which kernel
// family of a group ran: the tests of the kernel-selecting switches read it)
extern "C" const char* ds_routes(ds_ctx* c) {
    if (!c) return "";
    std::set<std::string> names;
    for (const char* n : c->routes) names.insert(n);
    c->routes.clear();
    c->routes_text.clear();
    for (auto& n : names) {
        if (!c->routes_text.empty()) c->routes_text += ' ';
        c->routes_text += n;
    }
    return c->routes_text.c_str();
}

// ---- internal helpers ------------------------------------------------------
static int get_twiddles(ds_ctx* c, int n, const float2** out);

// what reserve() allocates for a request of `bytes`: an eighth and 4 KB of room to grow into
static size_t reserved_bytes(size_t bytes) { return bytes + bytes / 8 + 4096; }

static int reserve(ds_ctx* c, void** buf, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return DS_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (*buf) HIPCHK(c, hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    const size_t want = reserved_bytes(bytes);
    hipError_t e = hipMalloc(buf, want);
    if (e != hipSuccess) return fail(c, DS_ERR_NOMEM, "workspace hipMalloc failed");
    *cap = want;
    return DS_OK;
}

// DS_ERR_NOMEM before anything is uploaded, for the families that promise it: the call will hold `ws` bytes of c->ws and
// `io` bytes of c->io as reserve() allocates them (1 MB each for the carves' 256-byte alignment) and `extra` bytes of
// its own allocations; what the two buffers hold now is given back first.
static int mem_check(ds_ctx* c, const char* who, size_t ws, size_t io, size_t extra) {
    const size_t need = reserved_bytes(ws + (1 << 20)) + reserved_bytes(io + (1 << 20)) + extra;
    size_t free_b = 0, total_b = 0;
    CHK(ds_mem_info(c, &free_b, &total_b));
    if (need > free_b + c->ws_bytes + c->io_bytes)
        return fail(c, DS_ERR_NOMEM, who, "the call needs more device memory than is free");
    return DS_OK;
}

struct Carver {  // 256-byte aligned sub-allocations out of one buffer; without a base it only adds up their sizes
    char* base = nullptr;
    size_t off = 0;
    Carver() = default;
    explicit Carver(void* b) : base((char*)b) {}
    template <typename T>
    T* take(size_t count) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
};

// The one place a buffer's pieces are written down: lay(Carver&) runs once to size *buf (grown by reserve), then
// again to place its pointers in it.  So lay takes pieces and stores the pointers; it launches, copies or fails nothing.
template <class F>
static int carve(ds_ctx* c, void** buf, size_t* cap, F&& lay) {
    Carver probe;
    lay(probe);
    CHK(reserve(c, buf, cap, probe.off));
    Carver cv(*buf);
    lay(cv);
    return DS_OK;
}

// One piece of c->ws or c->io: `count` elements of `elem` bytes, copied from the host array `src` once it is carved where
// one is given.  An optional piece the caller left out has count 0 or no src: it keeps its place and nothing is copied.
// `dst` is staged()'s: the host array the piece is copied to after the run.
struct Staged { size_t elem, count; const void* src = nullptr; void* dst = nullptr; };
static const size_t kMaxStaged = 12;

// The file's one carve-and-upload loop: carves the pieces out of *buf in list order, uploads those with a source and
// leaves the device address of piece i in d[i] (room for kMaxStaged).  The copies are synchronous: a source may be a
// local of the caller.
static int stage(ds_ctx* c, void** buf, size_t* cap, std::initializer_list<Staged> pieces, void** d) {
    const Staged* p = pieces.begin();
    const size_t n = pieces.size();
    if (n > kMaxStaged) return fail(c, DS_ERR_ARG, "stage: more than 12 pieces");
    CHK(carve(c, buf, cap, [&](Carver& cv) {
        for (size_t i = 0; i < n; ++i) d[i] = cv.take<char>(p[i].elem * p[i].count);
    }));
    for (size_t i = 0; i < n; ++i)
        if (p[i].src && p[i].count) CHK(ds_upload(c, d[i], p[i].src, p[i].elem * p[i].count));
    return DS_OK;
}

// How a host entry runs its device code (its _dev twin, or a runner they share).  The rule every entry follows: the
// caller's input and output arrays are pieces of c->io, staged here; tables and intermediates are pieces of c->ws,
// staged by stage() or carved by the device code itself -- so a host entry can call any _dev entry without the two
// overwriting each other.  staged() stages the pieces in c->io, calls run(d) with d[i] the device address of piece i and
// downloads the pieces that have a dst.  The entry validates before it calls this.
template <class F>
static int staged(ds_ctx* c, std::initializer_list<Staged> pieces, F&& run) {
    void* d[kMaxStaged];
    CHK(stage(c, &c->io, &c->io_bytes, pieces, d));
    CHK(run(d));
    for (const Staged& p : pieces)
        if (p.dst) CHK(ds_download(c, p.dst, d[&p - pieces.begin()], p.elem * p.count));
    return DS_OK;
}

static int prof_event(ds_ctx* c, hipEvent_t* ev) {
    if (!c->prof_pool.empty()) {
        *ev = c->prof_pool.back();
        c->prof_pool.pop_back();
        return DS_OK;
    }
    HIPCHK(c, hipEventCreate(ev));
    return DS_OK;
}

template <typename K, typename A>
static int launch(ds_ctx* c, const char* name, K kernel, dim3 grid, int threads, size_t lds,
                  const A& args) {
    if (lds > 64 * 1024)
        HIPCHK(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // "group@variant": the group is the name the profile reports (and ds_profile_only matches), the
    // whole string goes into the set ds_routes() hands out -- which kernel family really ran
    c->routes.insert(name);
    if (const char* at = strchr(name, '@')) {
        auto it = c->group_names.find(name);
        if (it == c->group_names.end()) it = c->group_names.emplace(name, std::string(name, at)).first;
        name = it->second.c_str();
    }
    ds_ctx::ProfRec rec{name, nullptr, nullptr};
    bool prof = c->prof && (c->prof_only.empty() || c->prof_only == name);
    if (prof && c->prof_stride > 1 && (c->prof_seen++ % c->prof_stride) != 0) prof = false;
    if (prof) {
        // The two events ride on the dispatch itself (hipExtLaunchKernel): they carry the kernel's own
        // begin / end timestamps -- what rocprofv3's kernel trace reports -- not the times of two marker
        // packets around it (hipEventRecord brackets held 4-6 us of dispatch and completion latency on top).
        CHK(prof_event(c, &rec.a));
        CHK(prof_event(c, &rec.b));
        hipExtLaunchKernelGGL(kernel, grid, dim3(threads), (std::uint32_t)lds, c->stream, rec.a, rec.b, 0u, args);
        HIPCHK(c, hipGetLastError());
        c->prof_recs.push_back(rec);
        return DS_OK;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, c->stream, args);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

// every Welch route ends here: chunk partials -> spectra / transfer functions (kernels_finish.hpp).  Partial slabs of
// 4 GiB or more leave the kernel's 32-bit raw-buffer descriptors (size_guards.hpp); DSPTOOLBOX_AMD_FINISH_WIDE=1
// sends every call down that 64-bit-load path (the GPU test of it: such slabs themselves do not fit a test).
// One thread per output value, 64 per workgroup.
static int launch_finish(ds_ctx* c, WelchFinArgs f) {
    const dim3 grid((unsigned)(((int64_t)f.fin.nb * (f.kind == 1 ? f.n_cx : f.n_cy) + 63) / 64));
    f.force_wide = c->cfg.finish_wide ? 1 : 0;
    const bool wide = f.force_wide || welch_finish_wide_slab((int64_t)f.n_cx * (f.in_nb > 0 ? f.in_nb : f.fin.nb),
                                                             (int64_t)f.n_cy * (f.in_nb > 0 ? f.in_nb : f.fin.nb));
    return launch(c, wide ? "welch_finish@wide" : "welch_finish", k_welch_finish, grid, 256, 0, f);
}

// The statements after OTHER with constexpr NN = n for the FFT lengths of the LDS-resident kernels; OTHER for any other n
#define DISPATCH_N_OR(n, OTHER, ...)                                               \
    switch (n) {                                                                   \
        case 8: { constexpr int NN = 8; __VA_ARGS__; } break;                      \
        case 16: { constexpr int NN = 16; __VA_ARGS__; } break;                    \
        case 32: { constexpr int NN = 32; __VA_ARGS__; } break;                    \
        case 64: { constexpr int NN = 64; __VA_ARGS__; } break;                    \
        case 128: { constexpr int NN = 128; __VA_ARGS__; } break;                  \
        case 256: { constexpr int NN = 256; __VA_ARGS__; } break;                  \
        case 512: { constexpr int NN = 512; __VA_ARGS__; } break;                  \
        case 1024: { constexpr int NN = 1024; __VA_ARGS__; } break;                \
        case 2048: { constexpr int NN = 2048; __VA_ARGS__; } break;                \
        case 4096: { constexpr int NN = 4096; __VA_ARGS__; } break;                \
        case 8192: { constexpr int NN = 8192; __VA_ARGS__; } break;                \
        case 16384: { constexpr int NN = 16384; __VA_ARGS__; } break;              \
        default: OTHER;                                                            \
    }
#define DISPATCH_N(n, ...) \
    DISPATCH_N_OR(n, return fail(c, DS_ERR_UNSUP, "FFT length must be a power of two in [8, 16384]"), __VA_ARGS__)

// The same for the few values of a runner's class count or flag: f(std::integral_constant<int, V>{}) for the V of Vs
// that v equals (every caller's v is one of them) / f(std::true_type{}) or f(std::false_type{})
template <int... Vs, class F>
static int dispatch(int v, F&& f) {
    int rc = DS_ERR_UNSUP;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}
template <class F> static int dispatch_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// per-length twiddle blob (fft_lds.hpp: one [k][t] table per pass, forward + reversed sequence)
static int get_twiddles(ds_ctx* c, int n, const float2** out) {
    auto it = c->tw.find(n);
    if (it != c->tw.end()) {
        *out = it->second;
        return DS_OK;
    }
    std::vector<float2> h;
    DISPATCH_N(n, {
        h.resize(std::max(1, tw_table_len<NN>()));
        fill_tw_table<NN>(h.data());
    });
    float2* d = nullptr;
    HIPCHK(c, hipMalloc((void**)&d, sizeof(float2) * h.size()));
    HIPCHK(c, hipMemcpyAsync(d, h.data(), sizeof(float2) * h.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tw[n] = d;
    *out = d;
    return DS_OK;
}

static int check_fft_len(ds_ctx* c, int n, const char* what) {
    if (!is_pow2(n) || n < kMinFft)
        return fail(c, DS_ERR_ARG, std::string(what) + ": length must be a power of two >= 8");
    if (n > kMaxFft)
        return fail(c, DS_ERR_UNSUP, std::string(what) + ": lengths above 16384 are not built yet (LDS-resident FFT)");
    return DS_OK;
}

// a context's constant table: filled on the host (fill(std::vector<float2>&)) and uploaded on first use
template <class Fill>
static int ensure_table(ds_ctx* c, float2** slot, Fill fill) {
    if (*slot) return DS_OK;
    std::vector<float2> h;
    fill(h);
    HIPCHK(c, hipMalloc((void**)slot, sizeof(float2) * h.size()));
    HIPCHK(c, hipMemcpyAsync(*slot, h.data(), sizeof(float2) * h.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DS_OK;
}
// twiddle tables of the wave-level transforms (stft1k::host_tables<N>), cached per context
template <int NN>
static int wave_tables(ds_ctx* c, const float2** out) {
    float2** tab = NN == 1024 ? &c->stft1k_tables : &c->stft_wave_tables[NN == 512 ? 0 : (NN == 256 ? 1 : 2)];
    CHK(ensure_table(c, tab, stft1k::host_tables<NN>));
    *out = *tab;
    return DS_OK;
}
// tables of the long-window transforms (R = length / 4096 classes, *lgR = log2 R): the 4096-point kernel's, then the
// radix-R stage's (*twl)
static int long_tables(ds_ctx* c, int R, int* lgR, const float2** twl) {
    for (*lgR = 0; (1 << *lgR) < R;) ++*lgR;
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    float2** slot = &c->wl_tables[*lgR - 1];
    CHK(ensure_table(c, slot, [R](std::vector<float2>& h) { welchl::host_tables(R, h); }));
    *twl = *slot;
    return DS_OK;
}
struct BigScratch {  // stft_big's scratch: two groups of four-step transforms and the frame means
    float2 *P, *Q;
    float* means;
};

// ---- four-step FFT for 2^15 .. 2^24 points (kernels_bigfft.hpp) -------------------
static int big_rows_ct(int n2) {
    int nt = dsfft::threads_for(n2);
    size_t per = (size_t)(((n2 + n2 / 16 + 2 + 30) / 32) * 32 + 1) * sizeof(float2);
    int ct = std::min<int>({16, 1024 / nt, std::max<int>(1, (int)((70 * 1024) / per))});
    while (ct & (ct - 1)) ct &= ct - 1;  // power of two: must divide N1
    return ct;
}

// cols stage of `batch` a.n_total-point transforms: k_big_cols<1024>, min(8, n2) columns per workgroup (sets n2, ct, tw)
static int launch_big_cols(ds_ctx* c, dsbig::ColsArgs a, int batch) {
    constexpr int N1 = 1024;
    a.n2 = (int)(a.n_total / N1);
    a.ct = std::min(8, a.n2);
    CHK(get_twiddles(c, N1, &a.tw));
    const size_t lds = (size_t)a.ct * dsbig::ch_stride<N1>() * sizeof(float2);
    return launch(c, "bigfft_cols", dsbig::k_big_cols<N1>, dim3(a.n2 / a.ct, batch), a.ct * Cfg<N1>::NT, lds, a);
}
// cols stage: source = complex `zin` (may equal `zout`) or real channel pairs
static int big_cols(ds_ctx* c, const float2* zin, const float* xreal, int n_ch, int64_t ld_real,
                    int64_t n_samples, float2* zout, int64_t N, int batch) {
    return launch_big_cols(c, {zin, xreal, nullptr, n_samples, 0, zout, N, 0, 0, 0, ld_real, n_ch, nullptr}, batch);
}

static int big_rows(ds_ctx* c, const float2* zin, float2* zout, int64_t N, int batch) {
    constexpr int N1 = 1024;
    const int n2 = (int)(N / N1);
    const float2* tw;
    CHK(get_twiddles(c, n2, &tw));
    const int ct = big_rows_ct(n2);
    dsbig::RowsArgs a{zin, zout, N, N1, ct, tw};
    size_t lds = 0;
    DISPATCH_N(n2, lds = (size_t)ct * dsbig::ch_stride<NN>() * sizeof(float2));
    DISPATCH_N(n2, CHK(launch(c, "bigfft_rows", dsbig::k_big_rows<NN>, dim3(N1 / ct, batch), ct * Cfg<NN>::NT, lds, a)));
    return DS_OK;
}

static int check_big_len(ds_ctx* c, int64_t n, const char* what) {
    if (!is_pow2(n)) return fail(c, DS_ERR_ARG, std::string(what) + ": internal: not a power of two");
    if (n > kMaxBigFft) return fail(c, DS_ERR_UNSUP, std::string(what) + ": lengths above 2^24 are not built yet");
    return DS_OK;
}

// ---- arbitrary lengths: Bluestein on top of the four-step FFT ------------------------
static int64_t blue_len(int64_t L) {
    int64_t m = (int64_t)1 << 15;  // smallest four-step length
    while (m < 2 * L - 1) m <<= 1;
    return m;
}

static int blue_filter(ds_ctx* c, int64_t L, int64_t M, const float2** out) {
    auto key = std::make_pair(L, M);
    auto it = c->blue.find(key);
    if (it != c->blue.end()) {
        it->second.stamp = ++c->blue_clock;
        *out = it->second.ptr;
        return DS_OK;
    }
    const size_t bytes = sizeof(float2) * (size_t)M;
    // make room: drop the least recently used tables (hipFree waits for the device, so a table
    // still referenced by queued kernels of an earlier call is never pulled from under them)
    while (!c->blue.empty() && c->blue_bytes + bytes > c->cfg.bluestein_cache_bytes) {
        auto lru = c->blue.begin();
        for (auto jt = c->blue.begin(); jt != c->blue.end(); ++jt)
            if (jt->second.stamp < lru->second.stamp) lru = jt;
        HIPCHK(c, hipFree(lru->second.ptr));
        c->blue_bytes -= lru->second.bytes;
        c->blue.erase(lru);
    }
    float2 *bt = nullptr, *bf = nullptr;
    HIPCHK(c, hipMalloc((void**)&bt, bytes));
    if (hipMalloc((void**)&bf, bytes) != hipSuccess) {
        (void)hipFree(bt);
        return fail(c, DS_ERR_NOMEM, "Bluestein filter table: hipMalloc failed");
    }
    int rc = DS_OK;
    do {
        hipLaunchKernelGGL(dsblue::k_filter, dim3(1024), dim3(256), 0, c->stream, bt, L, M);
        if (hipGetLastError() != hipSuccess) { rc = fail(c, DS_ERR_HIP, "Bluestein filter kernel launch failed"); break; }
        if ((rc = big_cols(c, bt, nullptr, 0, 0, 0, bt, M, 1)) != DS_OK) break;
        if ((rc = big_rows(c, bt, bf, M, 1)) != DS_OK) break;
        if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(c, DS_ERR_HIP, "Bluestein filter: stream sync failed"); break; }
    } while (0);
    (void)hipFree(bt);
    if (rc != DS_OK) {
        (void)hipFree(bf);
        return rc;
    }
    c->blue[key] = ds_ctx::BlueEntry{bf, bytes, ++c->blue_clock};
    c->blue_bytes += bytes;
    *out = bf;
    return DS_OK;
}

// X[batch][L] = DFT_L of (real channel pairs | complex zin[batch][L]); P, Q: [batch][M] scratch
static int blue_dft(ds_ctx* c, const float* xreal, int n_ch, int64_t ld_real, int64_t n_samples,
                    const float2* zin, int batch, int64_t L, int64_t M, float2* P, float2* Q, float2* X) {
    const float2* bf;
    CHK(blue_filter(c, L, M, &bf));
    dsblue::PreArgs pa{xreal, ld_real, n_samples, n_ch, zin, P, L, M};
    CHK(launch(c, "blue_pre", dsblue::k_pre, dim3(512, batch), 256, 0, pa));
    CHK(big_cols(c, P, nullptr, 0, 0, 0, P, M, batch));
    CHK(big_rows(c, P, Q, M, batch));
    hipLaunchKernelGGL(dsblue::k_mul_filter, dim3(512, batch), dim3(256), 0, c->stream, Q, bf, M);
    HIPCHK(c, hipGetLastError());
    CHK(big_cols(c, Q, nullptr, 0, 0, 0, Q, M, batch));
    CHK(big_rows(c, Q, P, M, batch));
    hipLaunchKernelGGL(dsblue::k_post, dim3(512, batch), dim3(256), 0, c->stream, (const float2*)P, X, L, M);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

static int check_blue_len(ds_ctx* c, int64_t L, const char* what) {
    if (L < 2) return fail(c, DS_ERR_ARG, std::string(what) + ": length must be >= 2");
    if (2 * L - 1 > kMaxBigFft) return fail(c, DS_ERR_UNSUP, std::string(what) + ": non-power-of-two lengths above 2^23 are not built yet");
    return DS_OK;
}

// ---- whole-signal rFFT, deconvolution ---------------------------------------
// One call of ds_rfft_dev (x -> spec) or ds_deconv_dev (y = x, r -> ir), checked by xform_check; `who`: the entry called
struct XformCall {
    const char* who;
    const float* x; int n_items, n_ch; int64_t ld, n_samples; int n_fft;
    float scale; float2* spec;                                             // rFFT
    const float2* r; int r_per_channel; int64_t n_out, ld_out; float* ir;  // deconvolution
};
static int xform_check(ds_ctx* c, const XformCall& q, bool deconv) {
    const std::string w(q.who), what = w + " n_fft";
    if (!c || !q.x || (deconv ? !q.r || !q.ir : !q.spec)) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_items <= 0 || q.n_ch <= 0 || q.n_samples <= 0 || q.ld < q.n_samples || q.n_samples > q.n_fft ||
        (deconv && (q.n_out <= 0 || q.n_out > q.n_fft || q.ld_out < q.n_out)))
        return fail(c, DS_ERR_ARG, w + (deconv ? ": bad shape" : ": bad shape (n_samples must be <= n_fft)"));
    if (!is_pow2(q.n_fft)) return check_blue_len(c, q.n_fft, what.c_str());
    if (q.n_fft > kMaxFft) return check_big_len(c, q.n_fft, what.c_str());
    return check_fft_len(c, q.n_fft, what.c_str());
}

// lengths that are not powers of two: Bluestein's DFT of the channel pairs, then (rFFT) the spectra unpacked, or
// (deconvolution) multiplied by r, transformed back and stored
static int xform_blue_run(ds_ctx* c, const XformCall& q) {
    const int npair = (q.n_ch + 1) / 2, batch = q.n_items * npair;
    const int64_t L = q.n_fft, M = blue_len(L);
    float2 *P, *Q, *X, *Y;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        P = cv.take<float2>((size_t)batch * M);
        Q = cv.take<float2>((size_t)batch * M);
        X = cv.take<float2>((size_t)batch * L);
        Y = q.spec ? nullptr : cv.take<float2>((size_t)batch * L);
    }));
    CHK(blue_dft(c, q.x, q.n_ch, q.ld, q.n_samples, nullptr, batch, L, M, P, Q, X));
    if (q.spec) {
        hipLaunchKernelGGL(dsblue::k_unpack, dim3(512, npair), dim3(256), 0, c->stream, (const float2*)X, L, q.n_ch,
                           q.scale, q.spec);
    } else {
        hipLaunchKernelGGL(dsblue::k_mul_r, dim3(512, batch), dim3(256), 0, c->stream, X, L, q.n_ch, q.r_per_channel, q.r);
        HIPCHK(c, hipGetLastError());
        CHK(blue_dft(c, nullptr, q.n_ch, 0, 0, X, batch, L, M, P, Q, Y));
        hipLaunchKernelGGL(dsblue::k_store, dim3(512, batch), dim3(256), 0, c->stream, (const float2*)Y, L, q.n_out,
                           q.ld_out, q.n_ch, q.ir);
    }
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}
// powers of two beyond the LDS-resident FFT: four-step transforms of the channel pairs, then (rFFT) the spectra
// unpacked, or (deconvolution) multiplied by r, transformed back and stored
static int xform_big_run(ds_ctx* c, const XformCall& q) {
    const int npair = (q.n_ch + 1) / 2, batch = q.n_items * npair;
    const int64_t N = q.n_fft;
    float2 *P, *Q;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        P = cv.take<float2>((size_t)batch * N);
        Q = cv.take<float2>((size_t)batch * N);
    }));
    CHK(big_cols(c, nullptr, q.x, q.n_ch, q.ld, q.n_samples, P, N, batch));
    CHK(big_rows(c, P, Q, N, batch));
    if (q.spec) {
        dsbig::UnpackArgs u{Q, N, q.n_ch, q.scale, q.spec, q.n_ch, 1};
        return launch(c, "bigfft_unpack", dsbig::k_big_unpack, dim3(1024, npair), 256, 0, u);
    }
    dsbig::MulArgs m{Q, N, q.n_ch, q.r_per_channel, q.r};
    CHK(launch(c, "bigfft_mul", dsbig::k_big_mul, dim3(1024, batch), 256, 0, m));
    CHK(big_cols(c, Q, nullptr, q.n_ch, 0, 0, Q, N, batch));
    CHK(big_rows(c, Q, P, N, batch));
    dsbig::StoreArgs st{P, N, q.n_out, q.ld_out, q.n_ch, q.ir};
    return launch(c, "bigfft_store", dsbig::k_big_store, dim3(1024, batch), 256, 0, st);
}
static int rfft_lds_run(ds_ctx* c, const XformCall& q) {
    const float2* tw;
    CHK(get_twiddles(c, q.n_fft, &tw));
    RfftArgs a{q.x, q.n_samples, q.ld, q.n_ch, tw, q.scale, q.spec};
    DISPATCH_N(q.n_fft, CHK(launch(c, "rfft", k_rfft<NN>, dim3((q.n_ch + 1) / 2), Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, a)));
    return DS_OK;
}

// 8192 points, one inverse spectrum for all channels: two register-resident 4096-point transforms per channel pair,
// the packed spectrum multiplied directly (kernels_deconv8k.hpp).
// Default since round 5: two persistent workgroups per CU, the next unit's samples in flight during this unit's
// transforms, the inverse spectrum from a permuted copy (k_rperm + k_deconv_p).  DSPTOOLBOX_AMD_DECONV_PERSIST=0 keeps
// one unit per workgroup: four workgroups per CU (k_deconv3q: all 1024 pairs of the benchmark resident at once), or
// three with DSPTOOLBOX_AMD_DECONV_4PERCU=0 (k_deconv3, 168 registers).  DSPTOOLBOX_AMD_DECONV_2PERCU=1 keeps the
// 512-thread kernel (A/B).
static int deconv8k_run(ds_ctx* c, const XformCall& q) {
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    CHK(ensure_table(c, &c->deconv8k_tables, deconv8k::host_tables));
    deconv8k::Args a8{q.x, q.n_samples, q.ld, q.n_out, q.ld_out, q.n_ch, c->w4_tables, c->deconv8k_tables, q.r, q.ir};
    const int64_t n_units = (int64_t)((q.n_ch + 1) / 2) * q.n_items;
    const bool two = c->cfg.deconv_2percu;
    // (n_units + grid stays an int inside the kernel: u + gridDim.x is formed for the prefetch past the last unit)
    if (c->cfg.deconv_persist && !two && n_units < ((int64_t)1 << 31) - 4096 && c->n_cu > 0) {
        if (!c->deconv_rperm) HIPCHK(c, hipMalloc((void**)&c->deconv_rperm, sizeof(float2) * deconv8k::RPERM_LEN));
        CHK(launch(c, "deconv_rperm", deconv8k::k_rperm, dim3(32), 256, 0, deconv8k::RpArgs{q.r, c->deconv_rperm}));
        deconv8k::PArgs pa{a8, c->deconv_rperm, (int)n_units};
        const int grid = (int)std::min<int64_t>(n_units, 2 * (int64_t)c->n_cu);
        return launch(c, "deconv@8k_persist", deconv8k::k_deconv_p, dim3((unsigned)grid), 256, deconv8k::LDS_BYTES_3, pa);
    }
    if (!two && c->cfg.deconv_4percu && n_units < ((int64_t)1 << 31))
        return launch(c, "deconv@8k_4percu", deconv8k::k_deconv3q, dim3((unsigned)n_units), 256, deconv8k::LDS_BYTES_3, a8);
    if (!two && n_units < ((int64_t)1 << 31))
        return launch(c, "deconv@8k_3percu", deconv8k::k_deconv3, dim3((unsigned)n_units), 256, deconv8k::LDS_BYTES_3, a8);
    return launch(c, "deconv@8k_512", deconv8k::k_deconv, dim3((q.n_ch + 1) / 2, q.n_items), deconv8k::NTB,
                  deconv8k::LDS_BYTES, a8);
}
static int deconv_generic_run(ds_ctx* c, const XformCall& q) {
    const float2* tw;
    CHK(get_twiddles(c, q.n_fft, &tw));
    DeconvArgs a{q.x, q.n_samples, q.ld, q.n_out, q.ld_out, q.n_ch, q.r_per_channel, tw, q.r, q.ir};
    const dim3 grid((q.n_ch + 1) / 2, q.n_items);
    DISPATCH_N(q.n_fft, CHK(launch(c, "deconv@generic", k_deconv<NN>, grid, Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, a)));
    return DS_OK;
}

using XformRunner = int (*)(ds_ctx*, const XformCall&);
// The kernel family of a checked call: Bluestein for lengths that are not powers of two, the four-step FFT beyond the
// LDS-resident one
static XformRunner rfft_route(const XformCall& q) {
    if (!is_pow2(q.n_fft)) return xform_blue_run;
    return q.n_fft > kMaxFft ? xform_big_run : rfft_lds_run;
}
static XformRunner deconv_route(const ds_ctx* c, const XformCall& q) {
    if (!is_pow2(q.n_fft)) return xform_blue_run;
    if (q.n_fft > kMaxFft) return xform_big_run;
    if (q.n_fft == deconv8k::N && !q.r_per_channel && !c->cfg.deconv_generic) return deconv8k_run;
    return deconv_generic_run;
}

extern "C" int ds_rfft_dev(ds_ctx* c, const float* x, int n_ch, int64_t ld, int64_t n_samples,
                           int n_fft, float scale, ds_c32* spec) {
    const XformCall q{"ds_rfft_dev", x, 1, n_ch, ld, n_samples, n_fft, scale, (float2*)spec};
    CHK(xform_check(c, q, false));
    return rfft_route(q)(c, q);
}

extern "C" int ds_deconv_inverse_dev(ds_ctx* c, const ds_c32* xspec, int n_ch, int n_bins,
                                     const float* eps, ds_c32* r) {
    if (!c || !xspec || !r || n_ch <= 0 || n_bins <= 0)
        return fail(c, DS_ERR_ARG, "ds_deconv_inverse: bad argument");
    int64_t total = (int64_t)n_ch * n_bins;
    hipLaunchKernelGGL(k_deconv_inverse, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                       (const float2*)xspec, n_ch, n_bins, eps, (float2*)r);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

extern "C" int ds_deconv_dev(ds_ctx* c, const float* y, int n_items, int n_ch, int64_t ld,
                             int64_t n_samples, int n_fft, const ds_c32* r, int r_per_channel,
                             int64_t n_out, int64_t ld_out, float* ir) {
    const XformCall q{"ds_deconv_dev", y, n_items, n_ch, ld, n_samples, n_fft, 1.0f, nullptr, (const float2*)r, r_per_channel,
                      n_out, ld_out, ir};
    CHK(xform_check(c, q, true));
    return deconv_route(c, q)(c, q);
}

// ---- STFT ------------------------------------------------------------------
// One call of ds_stft_r2c_dev, as every STFT runner takes it (checked by stft_check; `who`: the entry point called)
struct StftCall {
    const char* who;
    const float* x; int64_t n_samples; int n_ch; int64_t ld; int W, hop, nfft; int64_t pad_front; int n_frames;
    const float* window; int detrend; float scale, edge_scale; int power; float2* out;
};
static int stft_check(ds_ctx* c, const StftCall& s) {
    if (!c || !s.x || !s.out || !s.window) return fail(c, DS_ERR_ARG, s.who, "null argument");
    if (s.n_ch <= 0 || s.n_samples <= 0 || s.W <= 0 || s.hop <= 0 || s.n_frames <= 0 || s.ld < s.n_samples)
        return fail(c, DS_ERR_ARG, s.who, "bad shape");
    if (s.nfft < 2) return fail(c, DS_ERR_ARG, s.who, "fft length must be >= 2");
    return DS_OK;
}

// ---- framed transforms beyond the LDS-resident FFT (window / FFT length 2^15 .. 2^24) ------
// Frame pairs of every channel are one batch of four-step complex FFTs, processed in groups
// of <= 2^25 complex points per scratch buffer.
static int64_t stft_big_group(int64_t nfft, int64_t batch) {
    return std::max<int64_t>(1, std::min<int64_t>({batch, ((int64_t)1 << 25) / nfft, (int64_t)32768}));
}
static BigScratch take_big_scratch(Carver& cv, int n_ch, int n_frames, int64_t nfft) {
    const int64_t grp = stft_big_group(nfft, (int64_t)n_ch * ((n_frames + 1) / 2));
    BigScratch s;
    s.P = cv.take<float2>((size_t)grp * nfft);
    s.Q = cv.take<float2>((size_t)grp * nfft);
    s.means = cv.take<float>((size_t)n_ch * n_frames);
    return s;
}
// layout 0: out[(c*F + f)*nb + k] (unscaled spectra for the Welch sums), 1: out[(k*F + f)*C + c]
// s: take_big_scratch() for at least q.n_ch channels and q.n_frames frames
static int stft_big(ds_ctx* c, const BigScratch& s, const StftCall& q, int layout) {
    const int64_t nfft = q.nfft;
    CHK(check_big_len(c, nfft, "framed transform length"));
    const int64_t batch = (int64_t)q.n_ch * ((q.n_frames + 1) / 2);
    const int64_t grp = stft_big_group(nfft, batch);
    float2 *P = s.P, *Q = s.Q;
    float* means = s.means;
    if (q.detrend) {
        dsbig::FrameMeansArgs m{q.x, q.n_samples, q.ld, q.pad_front, q.n_ch, q.W, q.hop, q.n_frames, q.window, means};
        CHK(launch(c, "bigfft_means", dsbig::k_frame_means, dim3(q.n_frames, q.n_ch), 256, 0, m));
    }
    for (int64_t b0 = 0; b0 < batch; b0 += grp) {
        const int nb = (int)std::min<int64_t>(grp, batch - b0);
        CHK(launch_big_cols(c, {nullptr, q.x, nullptr, q.n_samples, 0, P, nfft, 0, 0, 0, q.ld, q.n_ch, nullptr, q.window,
                                q.detrend ? means : nullptr, q.W, q.hop, q.n_frames, q.pad_front, b0}, nb));
        CHK(big_rows(c, P, Q, nfft, nb));
        dsbig::UnpackFramesArgs u{Q, nfft, b0, q.n_ch, q.n_frames, layout, q.power, q.scale, q.edge_scale, q.out};
        CHK(launch(c, "bigfft_unpack", dsbig::k_big_unpack_frames, dim3(64, nb), 256, 0, u));
    }
    return DS_OK;
}
// the call for the unscaled spectra of q's whole windows (q: a WelchCall or a CsmCall), as the Welch and CSM sums take them
template <class Q>
static StftCall window_spectra(const Q& q, const float* x, int n_ch, int64_t ld, float2* out) {
    return {q.who, x, q.n_samples, n_ch, ld, q.W, q.hop, q.W, 0, q.n_frames, q.window, q.detrend, 1.0f, 1.0f, 0, out};
}

// any fft length (kernels_stft_any.hpp): rows = windowed frames -> ds_rfft_dev -> scaling pass
static int stft_any_run(ds_ctx* c, const StftCall& s) {
    const int nfft = s.nfft, keep = std::min(s.W, nfft), B = nfft / 2 + 1;
    const int64_t total_rows = (int64_t)s.n_frames * s.n_ch;
    // rows per group: the transform's scratch grows with the (padded) length; keep a group's
    // rows + spectra near 256 MB (Bluestein lengths count with their convolution length)
    int64_t conv = nfft;
    if (!is_pow2(nfft)) {
        conv = (int64_t)1 << 15;
        while (conv < 2 * (int64_t)nfft - 1) conv <<= 1;
    }
    int64_t group = std::max<int64_t>(2, ((int64_t)256 << 20) / (conv * 16));
    group = std::min<int64_t>(total_rows, group & ~(int64_t)1);
    if (group < 1) group = 1;
    float* rows;
    float2* tmp;
    CHK(carve(c, &c->aux, &c->aux_bytes, [&](Carver& cv) {
        rows = cv.take<float>((size_t)group * keep);
        tmp = cv.take<float2>((size_t)group * B);
    }));
    for (int64_t r0 = 0; r0 < total_rows; r0 += group) {
        const int nr = (int)std::min<int64_t>(group, total_rows - r0);
        stftany::PrepArgs pa{s.x, s.n_samples, s.ld, s.pad_front, s.n_ch, s.W, s.hop, s.detrend, s.window, keep, (int)r0, rows};
        CHK(launch(c, "stft_any_prepare", stftany::k_prepare, dim3(nr), 256, 0, pa));
        CHK(ds_rfft_dev(c, rows, nr, keep, keep, nfft, 1.0f, (ds_c32*)tmp));
        stftany::PostArgs po{tmp, s.out, B, nr, (int)r0, (int)total_rows, s.scale, s.edge_scale, (nfft % 2) == 0, s.power};
        const int64_t tot = (int64_t)B * nr;
        CHK(launch(c, "stft_any_post", stftany::k_post, dim3((unsigned)((tot + 255) / 256)), 256, 0, po));
    }
    return DS_OK;
}
// 2^15 ... 2^18 points: one decimation-in-frequency pass, then the 4096-point register transform per class
// (kernels_stft_long.hpp; k_sdif: frames of a group on grid.y, channel pairs on grid.z)
static int stft_long_run(ds_ctx* c, const StftCall& s) {
    const int R = stftl::classes_of(s.nfft);
    int lgR;
    const float2* twl;
    CHK(long_tables(c, R, &lgR, &twl));
    const int n_pc = (s.n_ch + 1) / 2, n_groups = (s.n_ch + 15) / 16;
    const int per = std::min(65535, stftl::frames_per_group(s.n_ch, s.nfft, s.n_frames));
    float2* b;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) { b = cv.take<float2>((size_t)n_pc * per * s.nfft); }));
    for (int f0 = 0; f0 < s.n_frames; f0 += per) {
        const int nf = std::min(per, s.n_frames - f0);
        // chunks of (frame, kind) units: two rounds of one workgroup (8 channels) per CU, as for 8192 / 16384 points
        const int n_units = nf * (R - 1);
        int n_chunks = std::max(1, std::min(n_units, 256 / std::max(1, std::min(256, n_groups))));
        if (c->cfg.stft4k_chunks > 0) n_chunks = std::min(n_units, c->cfg.stft4k_chunks);
        stftl::Args a{s.x, s.n_samples, s.ld, s.pad_front, s.n_ch, s.W, s.hop, s.n_frames, s.detrend, n_chunks, n_groups, R,
                      lgR, f0, nf, s.window, c->w4_tables, twl, s.scale, s.edge_scale, b, s.out};
        const dim3 gd(16, (unsigned)nf, (unsigned)n_pc), grid((unsigned)stft4k::grid_size(n_groups, n_chunks));
        CHK((dispatch<8, 16, 32, 64>(R, [&](auto r) { return launch(c, "stft_long_dif", stftl::k_sdif<r.value>, gd, 256, 0, a); })));
        CHK(dispatch_flag(s.power, [&](auto p) {
            return launch(c, "stft@long", stftl::k_stft_cls<p.value>, grid, stftl::NT, stftl::LDS_BYTES, a);
        }));
    }
    return DS_OK;
}
// powers of two beyond the register kernels: four-step transform per frame pair (kernels_bigfft.hpp)
static int stft_big_run(ds_ctx* c, const StftCall& s) {
    BigScratch b;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) { b = take_big_scratch(cv, s.n_ch, s.n_frames, s.nfft); }));
    return stft_big(c, b, s, 1);
}
// 256-, 512-, 1024- and 2048-point transforms (1024 = the reference's default frame): wave-level register transforms,
// one frame pair per team of NN / 16 lanes (kernels_stft1024.hpp).  Frames of 128 / 64 / 32 samples (NN = 256): their
// transform is every 2nd / 4th / 8th bin of the 256-point transform of the zero-padded frame (decim; removing the frame
// mean still only clears bin 0 of the kept bins)
static int stft_wave_run(ds_ctx* c, const StftCall& s) {
    return dispatch<256, 512, 1024, 2048>(s.nfft < 256 ? 256 : s.nfft, [&](auto n) {
        constexpr int NN = n.value;
        const float2* tab;
        CHK(wave_tables<NN>(c, &tab));
        // channels per workgroup: 16 teams = 128-byte runs of the output X[bin][frame][channel] (whole
        // cache lines; at 1024 points that is one 1024-thread workgroup of 140 KB per CU instead of two
        // of 8 channels with 64-byte runs: transform of the 64-microphone shape 105 -> 97 us);
        // 2048 points: 8 x 17 KB images, one 1024-thread workgroup per CU (4 channels = 32-byte runs,
        // two per CU: 0.20 ms against 0.16)
        const int lanes = NN / 16;
        int ct = std::min(NN >= 2048 ? 8 : 16, s.n_ch);
        if (const int v = c->cfg.stft_ct; v >= 1 && v <= 16 && v * lanes <= 1024) ct = std::min(v, s.n_ch);
        while (ct & (ct - 1)) ct &= ct - 1;
        const size_t lds = stft1k::lds_bytes<NN>(ct);
        const int threads = lanes * ct;
        // frame pairs per workgroup: as few as keep the whole grid resident at once, at most 16
        const int per_cu = std::max(1, std::min<int>({(int)((160 * 1024) / lds), 2048 / std::max(64, threads), 8}));
        const int n_fp = (s.n_frames + 1) / 2, n_ct = (s.n_ch + ct - 1) / ct;
        const int64_t resident = 256 * (int64_t)per_cu;
        int fpw = std::max(1, std::min(16, (int)(((int64_t)n_fp * n_ct + resident - 1) / resident)));
        if (c->cfg.stft_fpw > 0) fpw = c->cfg.stft_fpw;
        StftArgs a{s.x, s.n_samples, s.ld, s.pad_front, s.n_ch, s.W, s.hop, s.n_frames, s.detrend, s.power, ct, fpw, s.window,
                   tab, s.scale, s.edge_scale, s.out, NN / s.nfft};
        const dim3 grid((unsigned)((n_fp + fpw - 1) / fpw), (unsigned)n_ct);
        return dispatch_flag(s.power, [&](auto p) {
            return launch(c, "stft@wave", stft1k::k_stft_wave<NN, p.value>, grid, threads, lds, a);
        });
    });
}
// 4096-point transforms: the register-resident transform of the Welch path, four teams of two neighbouring
// channels per workgroup and frame (kernels_stft4096.hpp)
static int stft4k_run(ds_ctx* c, const StftCall& s) {
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    const int n_groups = (s.n_ch + 15) / 16;
    // chunks of frames: as many as put one workgroup (8 channels) on each of the 256 CUs
    int n_chunks = std::max(1, std::min(s.n_frames, 128 / std::max(1, std::min(128, n_groups))));
    if (c->cfg.stft4k_chunks > 0) n_chunks = std::min(s.n_frames, c->cfg.stft4k_chunks);
    stft4k::Args a{s.x, s.n_samples, s.ld, s.pad_front, s.n_ch, s.W, s.hop, s.n_frames, s.detrend, n_chunks, n_groups,
                   s.window, c->w4_tables, s.scale, s.edge_scale, s.out, nullptr};
    const dim3 grid((unsigned)stft4k::grid_size(n_groups, n_chunks));
    return dispatch_flag(s.power, [&](auto p) {
        return launch(c, "stft@4k", stft4k::k_stft<p.value>, grid, stft4k::NT, stft4k::LDS_BYTES, a);
    });
}
// 8192 / 16384 points: one radix-2 / radix-4 decimation-in-frequency stage on the windowed samples, then the
// 4096-point kernel's structure per residue (kernels_stft4096.hpp, k_stft_dif)
static int stft_dif_run(ds_ctx* c, const StftCall& s) {
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    float2** twn = &c->stft_dif_tw[s.nfft == 8192 ? 0 : 1];
    CHK(ensure_table(c, twn, [&s](std::vector<float2>& h) { stft4k::host_twiddles(s.nfft, h); }));
    const int n_groups = (s.n_ch + 15) / 16;
    // chunks of (frame, phase) units: two rounds of one workgroup (8 channels) per CU (64 x 512 000 samples, 8192
    // points: 0.182 ms against 0.198 with one round)
    int n_chunks = std::max(1, std::min(s.n_frames, 256 / std::max(1, std::min(256, n_groups))));
    if (c->cfg.stft4k_chunks > 0) n_chunks = std::min(s.n_frames, c->cfg.stft4k_chunks);
    stft4k::Args a{s.x, s.n_samples, s.ld, s.pad_front, s.n_ch, s.W, s.hop, s.n_frames, s.detrend, n_chunks, n_groups,
                   s.window, c->w4_tables, s.scale, s.edge_scale, s.out, *twn};
    const dim3 grid((unsigned)stft4k::grid_size(n_groups, n_chunks));
    return dispatch<2, 4>(s.nfft / 4096, [&](auto d) {
        return dispatch_flag(s.power, [&](auto p) {
            return launch(c, "stft@dif", stft4k::k_stft_dif<d.value, p.value>, grid, stft4k::NT, stft4k::Dif<d.value>::LDS_BYTES, a);
        });
    });
}
// every other power of two in [8, 16384]: the LDS-resident transform (kernels_generic.hpp)
static int stft_generic_run(ds_ctx* c, const StftCall& s) {
    const float2* tw;
    CHK(get_twiddles(c, s.nfft, &tw));
    // channel tile: ct teams of NT threads (<= 1024 threads, <= 74 KB of LDS so two
    // workgroups share a CU; 8 channels = 64-byte runs of the (bins, frames, channels) output for
    // nfft 1024: 0.16 ms instead of 0.23 ms with 4 on the 64-mic CSM shape)
    DISPATCH_N(s.nfft, {
        int ct = std::min<int>(stft_max_teams<NN>(), s.n_ch);
        // (override: fewer teams only, the kernel is compiled for the maximum)
        if (const int v = c->cfg.stft_ct; v >= 1 && v <= stft_max_teams<NN>()) ct = std::min(v, std::max(1, s.n_ch));
        while (ct & (ct - 1)) ct &= ct - 1;  // power of two (shift-only index math in the kernel)
        // frame pairs per workgroup: as few as keep the whole grid resident at once (two workgroups
        // on each of the 256 CUs: no second, partly filled round), at most 16
        const int n_fp = (s.n_frames + 1) / 2, n_ct = (s.n_ch + ct - 1) / ct;
        int fpw = std::max(1, std::min(16, (int)(((int64_t)n_fp * n_ct + 511) / 512)));
        if (c->cfg.stft_fpw > 0) fpw = c->cfg.stft_fpw;
        StftArgs a{s.x, s.n_samples, s.ld, s.pad_front, s.n_ch, s.W, s.hop, s.n_frames, s.detrend, s.power, ct, fpw,
                   s.window, tw, s.scale, s.edge_scale, s.out};
        CHK(launch(c, "stft@generic", k_stft<NN>, dim3((unsigned)((n_fp + fpw - 1) / fpw), (unsigned)n_ct), ct * Cfg<NN>::NT,
                   (size_t)stft_ch_stride<NN>() * sizeof(float2) * ct, a));
    });
    return DS_OK;
}
using StftRunner = int (*)(ds_ctx*, const StftCall&);
// The kernel family of a checked call: the register kernels of its length where they apply, the generic one otherwise.
static StftRunner stft_route(const ds_ctx* c, const StftCall& s) {
    const int nfft = s.nfft;
    if (!is_pow2(nfft) || nfft < kMinFft) return stft_any_run;  // numpy's rfft(n=...) takes any n: crop or pad
    // the register kernels: full frames, or shorter ones that are not detrended
    const bool reg = s.W <= nfft && (s.W == nfft || !s.detrend) && !c->cfg.stft_generic;
    if (stftl::classes_of(nfft) && reg && (s.n_ch + 1) / 2 <= 65535) return stft_long_run;
    if (nfft > kMaxFft) return stft_big_run;
    const int nfft_k = (nfft == 128 || nfft == 64 || nfft == 32) ? 256 : nfft;
    if ((nfft_k == 2048 || nfft_k == 1024 || nfft_k == 512 || nfft_k == 256) && reg &&
        stft1k::stft_wave_fits(s.n_samples, s.n_ch, s.ld, s.pad_front, nfft_k))
        return stft_wave_run;
    if (nfft == 4096 && reg && stft4k::fits(s.n_samples, s.pad_front)) return stft4k_run;
    if ((nfft == 8192 || nfft == 16384) && reg && stft4k::fits_long(s.n_samples, s.pad_front, nfft)) return stft_dif_run;
    return stft_generic_run;
}
extern "C" int ds_stft_r2c_dev(ds_ctx* c, const float* x, int64_t n_samples, int n_ch, int64_t ld,
                               int W, int hop, int nfft, int64_t pad_front, int n_frames,
                               const float* window, int detrend, float scale, float edge_scale,
                               int power, ds_c32* out) {
    const StftCall s{"ds_stft_r2c_dev", x, n_samples, n_ch, ld, W, hop, nfft, pad_front, n_frames, window, detrend,
                     scale, edge_scale, power, (float2*)out};
    CHK(stft_check(c, s));
    return stft_route(c, s)(c, s);
}

// ---- inverse STFT ----------------------------------------------------------
// One call of ds_istft_dev, as every iSTFT runner takes it (checked by istft_check; `who`: the entry point called)
struct IstftCall {
    const char* who;
    const float2* stft; int n_bins, n_frames, n_ch, nfft, W, step, frame_offset, n_frames_total; const float* window;
    float scale; int64_t total_length; float* out; int64_t ld_out;
};
static int istft_check(ds_ctx* c, const IstftCall& q) {
    if (!c || !q.stft || !q.window || !q.out) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_bins <= 0 || q.n_frames <= 0 || q.n_ch <= 0 || q.W <= 0 || q.step <= 0 || q.step > q.W || q.frame_offset < 0 ||
        q.n_frames_total < q.n_frames + q.frame_offset || q.total_length <= 0 || q.ld_out < q.total_length)
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (q.W > q.nfft) return fail(c, DS_ERR_ARG, q.who, "window longer than the FFT length");
    return DS_OK;
}
// overlap-add of the frames [c][f][W] into the output rows; four samples per thread (vec4) where every row and frame
// boundary is a multiple of four samples (and 16-byte aligned)
static int launch_ola(ds_ctx* c, const IstftCall& q, const float* frames, bool vec4) {
    IstftOlaArgs o{frames, q.n_frames, q.n_ch, q.W, q.step, q.frame_offset, q.n_frames_total, q.window, q.total_length,
                   q.ld_out, q.out};
    if (vec4 && q.W % 4 == 0 && q.step % 4 == 0 && q.total_length % 4 == 0 && q.ld_out % 4 == 0 &&
        ((uintptr_t)q.out & 15) == 0 && ((uintptr_t)q.window & 15) == 0)
        return launch(c, "istft_ola", k_istft_ola4, dim3((unsigned)((q.total_length / 4 + 255) / 256), q.n_ch), 256, 0, o);
    return launch(c, "istft_ola", k_istft_ola, dim3((unsigned)((q.total_length + 255) / 256), q.n_ch), 256, 0, o);
}
// 8192 ... 262144 points: class transforms on the 4096-point register kernel, then the radix-R stage with the
// overlap-add fused where frames overlap by half (kernels_istft_long.hpp)
static int istft_long_run(ds_ctx* c, const IstftCall& q) {
    const int R = istftl::classes_of(q.nfft);
    int lgR;
    const float2* twl;
    CHK(long_tables(c, R, &lgR, &twl));
    const int n_pc = (q.n_ch + 1) / 2, n_groups = (q.n_ch + 15) / 16;
    // (fused: the class sequences of ALL frames at once, addressed through a raw-buffer descriptor: below 4 GB)
    const bool fused = q.W == q.nfft && 2 * q.step == q.nfft && R <= 16 &&
                       (int64_t)n_pc * q.n_frames * q.nfft * 8 < ((int64_t)1 << 32) - 16;
    const int per = fused ? q.n_frames : istftl::frames_per_group(q.n_ch, q.nfft, q.n_frames);
    float2* cq;
    float* frames;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        cq = cv.take<float2>((size_t)n_pc * per * q.nfft);
        frames = fused ? nullptr : cv.take<float>((size_t)q.n_ch * q.n_frames * q.W);
    }));
    istftl::Args a{q.stft, q.n_bins, q.n_frames, q.n_ch, q.W, q.step, 1, n_groups, R, lgR, 0, q.n_frames, q.window,
                   c->w4_tables, twl, q.scale, cq, frames, q.frame_offset, q.n_frames_total, q.total_length, q.ld_out, q.out};
    for (int f0 = 0; f0 < q.n_frames; f0 += per) {
        a.f0 = f0;
        a.nf = std::min(per, q.n_frames - f0);
        const int n_units = a.nf * (R - 1);
        a.n_chunks = std::max(1, std::min(n_units, 256 / std::max(1, std::min(256, n_groups))));
        const dim3 gc((unsigned)stft4k::grid_size(n_groups, a.n_chunks));
        CHK(dispatch_flag((q.n_ch & 1) == 0, [&](auto p) {
            return launch(c, "istft_long_cls", istftl::k_icls<p.value>, gc, istftl::NT, istftl::LDS_BYTES, a);
        }));
        if (fused) break;
        const dim3 gd(16, (unsigned)a.nf, (unsigned)n_pc);
        CHK((dispatch<2, 4, 8, 16, 32, 64>(R, [&](auto r) {
            return launch(c, "istft@long", istftl::k_isdif_frames<r.value>, gd, 256, istftl::xch_bytes(r.value), a);
        })));
    }
    if (!fused) return launch_ola(c, q, frames, true);
    // chunks of frames (+ 1 frame each for the carry): 8192 workgroups of 256 threads where the frames allow
    // (a thread has only R loads in flight), at least 4 frames per chunk
    const int want = std::max(1, 8192 / std::max(1, 16 * n_pc));
    a.n_chunks = std::max(1, std::min((q.n_frames + 3) / 4, want));
    if (c->cfg.istft_fpw > 0) a.n_chunks = std::min(q.n_frames, c->cfg.istft_fpw);
    const dim3 gd(16, (unsigned)a.n_chunks, (unsigned)n_pc);
    return dispatch<2, 4, 8, 16>(R, [&](auto r) {
        return launch(c, "istft@long_ola", istftl::k_isdif_ola<r.value>, gd, 256, istftl::xch_bytes(r.value), a);
    });
}

// ---- inverse STFT with an FFT length that is not a power of two (transforms/transforms.py:548-577 calls
// np.fft.irfft(stft, n=fft_length_samples) with any n) ------------------------------------------------------
// Every (channel, frame) spectrum is one "channel" of the spectral-division machinery, which already
// inverts any length (Bluestein on the four-step transform): irfft_n(1 * R) with a unit impulse as the
// numerator.  k_istft_spec lays the spectra out per (channel, frame) -- cropped or zero-padded to
// n / 2 + 1 bins as numpy does --, the division writes the frames [c][f][W], k_istft_scale applies the
// synthesis window and the scale; the overlap-add kernel is the same as for powers of two.
__global__ void k_istft_spec(const float2* stft, int n_bins, int n_frames, int n_ch, int f0, int nf, int nb, float2* r,
                             float* ones) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, total = (int64_t)n_ch * nf * nb;
    if (i < (int64_t)n_ch * nf) ones[i] = 1.f;
    if (i >= total) return;
    const int k = (int)(i % nb);
    const int64_t cf = i / nb;
    const int f = (int)(cf % nf), ch = (int)(cf / nf);
    r[i] = k < n_bins ? stft[((int64_t)k * n_frames + f0 + f) * n_ch + ch] : make_float2(0.f, 0.f);
}
__global__ void k_istft_scale(float* frames, int64_t total, int W, const float* window, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) frames[i] *= scale * window[i % W];
}
static int istft_any_run(ds_ctx* c, const IstftCall& q) {
    const int n_ch = q.n_ch, n_frames = q.n_frames, nfft = q.nfft, W = q.W;
    // (ws, io and aux are all taken -- the division's scratch, the host entry point's staging, the
    // per-group spectra -- so the frames live in a fourth context-owned reserve: grown on demand like
    // the others, no allocation, synchronisation or free per call; this route is correct, not tuned)
    CHK(reserve(c, &c->frames, &c->frames_bytes, sizeof(float) * (size_t)n_ch * n_frames * W));
    float* frames = (float*)c->frames;  // [c][f][W]
    CHK(check_blue_len(c, nfft, (std::string(q.who) + " nfft").c_str()));
    const int nb = nfft / 2 + 1;
    // groups of frames: the division's scratch is ~4 x 8 bytes x (frames x channels / 2) x transform length
    const int64_t m_len = blue_len(nfft);
    int group = (int)std::max<int64_t>(1, ((int64_t)64 << 20) / std::max<int64_t>(1, m_len * n_ch));
    group = std::min(group, n_frames);
    float2* r;
    float *ones, *part;
    CHK(carve(c, &c->aux, &c->aux_bytes, [&](Carver& cv) {
        r = cv.take<float2>((size_t)n_ch * group * nb);
        ones = cv.take<float>((size_t)n_ch * group);
        part = cv.take<float>((size_t)n_ch * group * W);
    }));
    for (int f0 = 0; f0 < n_frames; f0 += group) {
        const int nf = std::min(group, n_frames - f0);
        const int64_t total = (int64_t)n_ch * nf * nb;
        hipLaunchKernelGGL(k_istft_spec, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, q.stft, q.n_bins,
                           n_frames, n_ch, f0, nf, nb, r, ones);
        HIPCHK(c, hipGetLastError());
        CHK(ds_deconv_dev(c, ones, 1, n_ch * nf, 1, 1, nfft, (const ds_c32*)r, 1, W, W, part));
        // part: [(ch nf + f) W + m] -> frames [(ch n_frames + f0 + f) W + m], windowed and scaled
        const int64_t tw = (int64_t)n_ch * nf * W;
        // (`scale` is defined against an UNnormalised inverse transform, as k_istft computes it; the division
        // machinery returns numpy's normalised irfft)
        hipLaunchKernelGGL(k_istft_scale, dim3((unsigned)((tw + 255) / 256)), dim3(256), 0, c->stream, part, tw, W, q.window,
                           q.scale * (float)nfft);
        HIPCHK(c, hipGetLastError());
        for (int ch = 0; ch < n_ch; ++ch)
            HIPCHK(c, hipMemcpyAsync(frames + ((int64_t)ch * n_frames + f0) * W, part + (int64_t)ch * nf * W,
                                     sizeof(float) * (size_t)nf * W, hipMemcpyDeviceToDevice, c->stream));
    }
    return launch_ola(c, q, frames, false);
}
// The fused runners below: 50 % overlap of full-length frames, transform and overlap-add in one kernel, no frames in
// memory.  Every power-of-two route in [8, 16384] uploads the generic twiddles of its length first, used or not.
// ... on the wave-level transform for 256 ... 2048 points (kernels_stft1024.hpp, k_istft_wave)
static int istft_wave_run(ds_ctx* c, const IstftCall& q) {
    return dispatch<256, 512, 1024, 2048>(q.nfft, [&](auto n) {
        constexpr int NN = n.value;
        const float2 *tw, *tab;
        CHK(get_twiddles(c, NN, &tw));
        CHK(wave_tables<NN>(c, &tab));
        // (2048 points: 45 registers over the 128 of a 1024-thread workgroup: four teams = 512 threads there)
        const int lanes = NN / 16;
        int ct = std::min(NN == 2048 ? 4 : 16, q.n_ch);
        while (ct & (ct - 1)) ct &= ct - 1;
        const size_t lds = stft1k::istft_lds_bytes<NN>(ct);
        const int threads = lanes * ct;
        const int n_fp = (q.n_frames + 1) / 2, n_ct = (q.n_ch + ct - 1) / ct;
        const int per_cu = std::max(1, std::min<int>((int)((160 * 1024) / lds), 2048 / std::max(64, threads)));
        // frame pairs per workgroup (+ 1 for the carry): two rounds of resident workgroups, at least 4 (1024 points: 8)
        // -- 64 x 512 000 samples: 0.154 / 0.130 / 0.135 ms at 256 / 512 / 1024 points, 0.18 / 0.13 / 0.145 one step off
        int fpw = std::max(NN >= 1024 ? 8 : 4, std::min(64, (int)(((int64_t)n_fp * n_ct + 512 * per_cu - 1) / (512 * per_cu))));
        if (c->cfg.istft_fpw > 0) fpw = c->cfg.istft_fpw;
        IstftFusedArgs fa{IstftArgs{q.stft, q.n_bins, q.n_frames, q.n_ch, q.W, q.window, tab, q.scale, nullptr, ct, fpw},
                          q.frame_offset, q.n_frames_total, q.total_length, q.ld_out, q.out};
        const dim3 grid((unsigned)((n_fp + fpw - 1) / fpw), (unsigned)n_ct);
        return launch(c, "istft@wave", stft1k::k_istft_wave<NN>, grid, threads, lds, fa);
    });
}
// ... on the 4096-point register transform, two neighbouring channels per team (kernels_stft4096.hpp, k_istft)
static int istft4k_run(ds_ctx* c, const IstftCall& q) {
    const float2* tw;
    CHK(get_twiddles(c, q.nfft, &tw));
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    const int n_groups = (q.n_ch + 15) / 16;
    // chunks of frames (+ 1 frame each for the carry): two rounds of one workgroup (8 channels) per CU
    int n_chunks = std::max(1, std::min((q.n_frames + 3) / 4, 256 / std::max(1, std::min(256, n_groups))));
    if (c->cfg.istft_fpw > 0) n_chunks = std::min(q.n_frames, c->cfg.istft_fpw);
    IstftFusedArgs fa{IstftArgs{q.stft, q.n_bins, q.n_frames, q.n_ch, q.W, q.window, c->w4_tables, q.scale, nullptr, 1, n_chunks},
                      q.frame_offset, q.n_frames_total, q.total_length, q.ld_out, q.out};
    const dim3 g4((unsigned)stft4k::grid_size(n_groups, n_chunks));
    return dispatch_flag((q.n_ch & 1) == 0, [&](auto p) {
        return launch(c, "istft@4k", stft4k::k_istft<p.value>, g4, stft4k::NT, stft4k::ISTFT_LDS_BYTES, fa);
    });
}
// ... and on the LDS-resident transform where it has more than one team and whole 2 NT-point steps (kernels_generic.hpp)
template <int NN> static constexpr bool istft_fuses() { return stft_max_teams<NN>() > 1 && NN % (2 * Cfg<NN>::NT) == 0; }
static int istft_fused_run(ds_ctx* c, const IstftCall& q) {
    const float2* tw;
    CHK(get_twiddles(c, q.nfft, &tw));
    DISPATCH_N(q.nfft, if constexpr (istft_fuses<NN>()) {
        int ct = std::min<int>(stft_max_teams<NN>(), q.n_ch);
        while (ct & (ct - 1)) ct &= ct - 1;
        const size_t lds = (size_t)stft_ch_stride<NN>() * sizeof(float2) * ct + sizeof(float) * (size_t)(NN / 2);  // + 1 / envelope
        const int n_fp = (q.n_frames + 1) / 2, n_ct = (q.n_ch + ct - 1) / ct;
        // frame pairs per workgroup: every workgroup transforms one more pair (the carry in front of its range)
        // (64 x 512 000 samples, windows of 256 / 1024 / 4096: ~250 workgroups measured best: 0.21 / 0.21 / 0.29 ms)
        int fpw = std::max(4, std::min(64, (int)(((int64_t)n_fp * n_ct + 255) / 256)));
        if (c->cfg.istft_fpw > 0) fpw = c->cfg.istft_fpw;
        IstftFusedArgs fa{IstftArgs{q.stft, q.n_bins, q.n_frames, q.n_ch, q.W, q.window, tw, q.scale, nullptr, ct, fpw},
                          q.frame_offset, q.n_frames_total, q.total_length, q.ld_out, q.out};
        CHK(launch(c, "istft@fused", k_istft_fused<NN>, dim3((unsigned)((n_fp + fpw - 1) / fpw), (unsigned)n_ct),
                   ct * Cfg<NN>::NT, lds, fa));
    });
    return DS_OK;
}
// Every other power of two in [8, 16384]: the frames into the workspace, then the overlap-add.  ct neighbouring
// channels per workgroup (runs of 8 ct bytes of the channel-fastest spectrogram) wherever more than one image fits;
// DSPTOOLBOX_AMD_ISTFT_CT=1 keeps one channel per workgroup
static int istft_frames_run(ds_ctx* c, const IstftCall& q) {
    const float2* tw;
    CHK(get_twiddles(c, q.nfft, &tw));
    CHK(reserve(c, &c->ws, &c->ws_bytes, sizeof(float) * (size_t)q.n_ch * q.n_frames * q.W));
    float* frames = (float*)c->ws;
    IstftArgs a{q.stft, q.n_bins, q.n_frames, q.n_ch, q.W, q.window, tw, q.scale, frames};
    DISPATCH_N(q.nfft, {
        int ct = std::min<int>(stft_max_teams<NN>(), q.n_ch);
        while (ct & (ct - 1)) ct &= ct - 1;
        if (ct == 1 || c->cfg.istft_one_ch) {
            CHK(launch(c, "istft@generic", k_istft<NN>, dim3((q.n_frames + 1) / 2, q.n_ch), Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, a));
        } else if constexpr (stft_max_teams<NN>() > 1) {
            const int n_fp = (q.n_frames + 1) / 2, n_ct = (q.n_ch + ct - 1) / ct;
            a.ct = ct;
            a.fpw = std::max(1, std::min(16, (int)(((int64_t)n_fp * n_ct + 511) / 512)));
            CHK(launch(c, "istft@ct", k_istft_ct<NN>, dim3((unsigned)((n_fp + a.fpw - 1) / a.fpw), (unsigned)n_ct),
                       ct * Cfg<NN>::NT, (size_t)stft_ch_stride<NN>() * sizeof(float2) * ct, a));
        }
    });
    return launch_ola(c, q, frames, true);
}
using IstftRunner = int (*)(ds_ctx*, const IstftCall&);
// The kernel family of a checked call, in the order the routes were written down: the long-window classes, any
// length, the fused kernels at 50 % overlap of full frames, the two-launch path.
static IstftRunner istft_route(const ds_ctx* c, const IstftCall& q) {
    const int nfft = q.nfft;
    const bool fused = c->cfg.istft_fused, wave = c->cfg.istft_wave;
    // (the spectrogram through a raw-buffer descriptor: below 4 GiB)
    const bool spec_fits = (int64_t)q.n_bins * q.n_frames * q.n_ch * 8 < ((int64_t)1 << 32) - 16;
    if (istftl::classes_of(nfft) && wave && fused && q.n_frames <= 65535 && (q.n_ch + 1) / 2 <= 65535 && spec_fits)
        return istft_long_run;
    if (!is_pow2(nfft) || nfft < kMinFft || nfft > kMaxFft) return istft_any_run;
    const bool half = q.W == nfft && 2 * q.step == nfft && q.n_ch > 1 && fused;
    // (the wave kernels' team count, min(16, n_ch) or at 2048 points min(4, n_ch), is > 1 wherever n_ch > 1)
    if (half && wave && (nfft == 2048 || nfft == 1024 || nfft == 512 || nfft == 256) && spec_fits) return istft_wave_run;
    if (half && nfft == 4096 && wave && q.total_length < ((int64_t)1 << 31) && spec_fits) return istft4k_run;
    bool fuses = false;  // (its team count min(stft_max_teams, n_ch) is > 1 wherever stft_max_teams and n_ch are)
    DISPATCH_N_OR(nfft, break, fuses = istft_fuses<NN>());
    return half && fuses ? istft_fused_run : istft_frames_run;
}
extern "C" int ds_istft_dev(ds_ctx* c, const ds_c32* stft, int n_bins, int n_frames, int n_ch, int nfft,
                            int W, int step, int frame_offset, int n_frames_total, const float* window,
                            float scale, int64_t total_length, float* out, int64_t ld_out) {
    const IstftCall q{"ds_istft_dev", (const float2*)stft, n_bins, n_frames, n_ch, nfft, W, step, frame_offset,
                      n_frames_total, window, scale, total_length, out, ld_out};
    CHK(istft_check(c, q));
    return istft_route(c, q)(c, q);
}

// ---- band powers of a spectrogram (mel spectrogram / MFCC) ----------------------------------
// what ds_band_power and its _dev twin both refuse (the pointers are the host's or the device's)
static int band_power_check(ds_ctx* c, const void* stft, const void* weights, const void* band_start, const void* band_stop,
                            const void* out, int n_bins, int64_t n_fc, int n_bands) {
    if (!c || !stft || !weights || !band_start || !band_stop || !out)
        return fail(c, DS_ERR_ARG, "ds_band_power: null argument");
    if (n_bins <= 0 || n_fc <= 0 || n_bands <= 0) return fail(c, DS_ERR_ARG, "ds_band_power: bad shape");
    return DS_OK;
}

extern "C" int ds_band_power_dev(ds_ctx* c, const ds_c32* stft, int n_bins, int64_t n_fc, const float* weights,
                                 const int* band_start, const int* band_stop, int n_bands, int to_db,
                                 int dct_abs, float* out) {
    CHK(band_power_check(c, stft, weights, band_start, band_stop, out, n_bins, n_fc, n_bands));
    if (n_bands > 65535) return fail(c, DS_ERR_ARG, "ds_band_power: bad shape");  // (the grid's y extent)
    float* dst = out;
    if (dct_abs) {
        CHK(reserve(c, &c->ws, &c->ws_bytes, sizeof(float) * (size_t)n_bands * n_fc));
        dst = (float*)c->ws;
    }
    BandPowerArgs a{(const float2*)stft, weights, band_start, band_stop, n_bins, n_bands, n_fc, to_db, dst};
    const unsigned gx = (unsigned)((n_fc + 255) / 256);
    CHK(launch(c, "band_power", k_band_power, dim3(gx, n_bands), 256, 0, a));
    if (dct_abs) {
        DctArgs d{dst, n_bands, n_fc, out};
        CHK(launch(c, "dct2_abs", k_dct2_abs, dim3(gx, n_bands), 256, 0, d));
    }
    return DS_OK;
}

extern "C" int ds_band_power(ds_ctx* c, const ds_c32* stft, int n_bins, int64_t n_fc, const float* weights,
                             const int* band_start, const int* band_stop, int n_bands, int to_db, int dct_abs,
                             float* out) {
    CHK(band_power_check(c, stft, weights, band_start, band_stop, out, n_bins, n_fc, n_bands));
    const size_t ns = (size_t)n_bins * n_fc, nw = (size_t)n_bands * n_bins, no = (size_t)n_bands * n_fc, nbd = n_bands;
    return staged(c, {{8, ns, stft, nullptr}, {4, nw, weights, nullptr}, {4, nbd, band_start, nullptr},
                      {4, nbd, band_stop, nullptr}, {4, no, nullptr, out}},
                  [&](void* const* d) {
                      return ds_band_power_dev(c, (const ds_c32*)d[0], n_bins, n_fc, (const float*)d[1], (const int*)d[2],
                                               (const int*)d[3], n_bands, to_db, dct_abs, (float*)d[4]);
                  });
}

// ---- Welch -----------------------------------------------------------------
struct WelchPlan {
    int n_chunks, fpc;
};
static WelchPlan plan_welch(int n_frames, int units) {
    // >= ~1024 workgroups when there is enough work, <= 32 frames per fp32 chain
    int by_len = (n_frames + 31) / 32;
    int by_fill = (1024 + units - 1) / units;
    int n_chunks = std::max(by_len, std::min(by_fill, (n_frames + 1) / 2));
    n_chunks = std::max(1, n_chunks);
    int fpc = (n_frames + n_chunks - 1) / n_chunks;
    fpc = (fpc + 1) & ~1;  // even: frames travel in pairs in the input-spectra kernel
    n_chunks = (n_frames + fpc - 1) / fpc;
    return {n_chunks, fpc};
}

// What a Welch call estimates; the values are kernel arguments (k_welch_finish, k_welch_median, dsbig::k_spec_sum)
enum WelchKind { TF = 0, PSD = 1, CSD = 2 };
// One call of a Welch entry, as every Welch runner takes it (checked by welch_check; `who`: the entry point called).
// TF: transfer function and coherence of y against x (out_c, out_r); PSD: auto spectra of x (out_r; y and out_c null,
// n_cy = ldy = mode = 0); CSD: cross spectra conj(X_c) Y_c (out_c; out_r null, mode 0)
struct WelchCall {
    const char* who;
    WelchKind kind;
    const float* x; int n_cx; int64_t ldx; const float* y; int n_cy; int64_t ldy, n_samples; int W, hop, n_frames;
    const float* window; int detrend, average, mode, amp_sqrt; double norm_scale, factor; int halve_edges;
    float2* out_c; float* out_r;
    bool auto_only() const { return kind == PSD; }
    int n_out() const { return auto_only() ? n_cx : n_cy; }  // channels that are accumulated
    int nyc() const { return auto_only() ? 0 : n_cy; }       // channels of y that are transformed
    bool big() const { return W > kMaxFft && is_pow2(W); }   // window beyond the LDS-resident FFT: four-step transforms
};
// What every Welch runner hands to launch_finish: the partial slabs of n_chunks chunks and nb bins (pxx: of the input
// channels; auto spectra: of x), scaled for the mean over the call's frames
static WelchFinArgs welch_fin(const WelchCall& q, const float* pxx, const float2* pxy, const float* pyy, int n_chunks, int nb) {
    return {pxx, pxy, pyy, n_chunks, n_chunks, q.n_cx, q.n_cy, q.kind, q.mode,
            FinishPar{q.norm_scale / (double)q.n_frames, q.factor, q.halve_edges, q.amp_sqrt, nb}, q.out_c, q.out_r};
}
// a register kernel's arguments for the y signal: those of x with y's samples, row stride and channel count
template <class A>
static A y_args(A a, const WelchCall& q) {
    a.sig = q.y;
    a.ld = q.ldy;
    a.n_ch = q.n_cy;
    return a;
}

// Median kernels keep `series` float series of n_frames values (padded to a power of two) per bin in LDS: the number of bins
// per workgroup (8, 4, 2 or 1) that fits 150 KB; 0 if not even one does.
static int median_bins_per_block(int series, int n_frames, size_t* lds) {
    for (int bpb = 8; bpb >= 1; bpb >>= 1) {
        const size_t need = ((size_t)bpb * series * median_stride(n_frames) + (size_t)bpb * series * 2) * sizeof(float);
        if (need <= 150 * 1024) {
            *lds = need;
            return bpb;
        }
    }
    return 0;
}

// Welch for window lengths beyond the LDS-resident FFT: spectra of every frame -> frame sums
// (or per-bin medians) -> the usual finish
static int welch_big_run(ds_ctx* c, const WelchCall& q) {
    const int n_cx = q.n_cx, n_frames = q.n_frames, nb = q.W / 2 + 1;
    const int nyc = q.nyc();
    const int nmax = std::max(n_cx, nyc);
    size_t med_lds = 0;
    const int med_bpb = median_bins_per_block(3, n_frames, &med_lds);
    if (q.average == DS_AVG_MEDIAN && !med_bpb)
        return fail(c, DS_ERR_UNSUP, "welch: median averaging over more than 12 799 frames is not built yet");
    float2 *xsp, *ysp, *pxy;
    float *pxx, *pyy;
    BigScratch s;  // the FFT scratch is reused by both signals
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        xsp = cv.take<float2>((size_t)n_cx * n_frames * nb);
        ysp = cv.take<float2>((size_t)std::max(1, nyc) * n_frames * nb);
        pxx = cv.take<float>((size_t)n_cx * nb);
        pxy = cv.take<float2>((size_t)std::max(1, nyc) * nb);
        pyy = cv.take<float>((size_t)std::max(1, nyc) * nb);
        s = take_big_scratch(cv, nmax, n_frames, q.W);
    }));
    CHK(stft_big(c, s, window_spectra(q, q.x, n_cx, q.ldx, xsp), 0));
    if (nyc) CHK(stft_big(c, s, window_spectra(q, q.y, nyc, q.ldy, ysp), 0));
    WelchFinArgs f = welch_fin(q, pxx, pxy, pyy, 1, nb);
    if (q.average == DS_AVG_MEDIAN) {
        MedianArgs m{xsp, nyc ? ysp : nullptr, n_cx, nyc, n_frames, nb, q.kind, med_bpb, pxx, pxy, pyy};
        CHK(launch(c, "welch_median", k_welch_median, dim3((nb + med_bpb - 1) / med_bpb, q.n_out()), 256, med_lds, m));
        const int nbias = (n_frames & 1) ? n_frames : n_frames - 1;
        const double count = 1.0 / (double)std::max(1, nbias);
        f.fin.inv = q.norm_scale / count;
    } else {
        dsbig::SpecSumArgs sa{xsp, nyc ? ysp : nullptr, n_cx, nyc, n_frames, nb, q.kind, pxx, pxy, pyy};
        CHK(launch(c, "welch_specsum", dsbig::k_spec_sum, dim3((nb + 255) / 256, q.n_out()), 256, 0, sa));
    }
    return launch_finish(c, f);
}

// Median averaging for windows up to 16384 samples: frame spectra of x (and y) -> per-bin medians -> the usual finish
// with bias n (n = F or F-1, odd; the reference's `csd /= sum((-1)**(n+1)/n)` multiplies by n)
static int welch_median_run(ds_ctx* c, const WelchCall& q) {
    const int n_cx = q.n_cx, n_frames = q.n_frames, W = q.W;
    CHK(check_fft_len(c, W, "welch window length"));
    const float2* tw;
    CHK(get_twiddles(c, W, &tw));
    const int nb = W / 2 + 1;
    WelchPlan pl = plan_welch(n_frames, q.auto_only() ? n_cx : (q.n_cy + 1) / 2);
    const int nyc = q.nyc();
    size_t lds = 0;
    const int bpb = median_bins_per_block(3, n_frames, &lds);
    if (!bpb)
        return fail(c, DS_ERR_UNSUP, "welch: median averaging over more than 12 799 frames is not built yet");
    float2 *xsp, *ysp, *mxy;
    float *scratch, *mxx, *myy;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        xsp = cv.take<float2>((size_t)n_cx * n_frames * nb);
        ysp = nyc ? cv.take<float2>((size_t)nyc * n_frames * nb) : nullptr;
        scratch = cv.take<float>((size_t)pl.n_chunks * std::max(n_cx, nyc) * nb);
        mxx = cv.take<float>((size_t)n_cx * nb);
        mxy = cv.take<float2>((size_t)std::max(1, nyc) * nb);
        myy = cv.take<float>((size_t)std::max(1, nyc) * nb);
    }));
    {
        XspecArgs ax{q.x, q.n_samples, q.ldx, n_cx, W, q.hop, n_frames, q.detrend, pl.fpc, q.window, tw, xsp, scratch};
        DISPATCH_N(W, CHK(launch(c, "welch_xspec", k_xspec<NN>, dim3(pl.n_chunks, n_cx), Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, ax)));
    }
    if (nyc) {
        XspecArgs ay{q.y, q.n_samples, q.ldy, nyc, W, q.hop, n_frames, q.detrend, pl.fpc, q.window, tw, ysp, scratch};
        DISPATCH_N(W, CHK(launch(c, "welch_xspec", k_xspec<NN>, dim3(pl.n_chunks, nyc), Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, ay)));
    }
    MedianArgs m{xsp, ysp, n_cx, nyc, n_frames, nb, q.kind, bpb, mxx, mxy, myy};
    CHK(launch(c, "welch_median", k_welch_median, dim3((nb + bpb - 1) / bpb, q.n_out()), 256, lds, m));
    const int nbias = (n_frames & 1) ? n_frames : n_frames - 1;
    WelchFinArgs f = welch_fin(q, mxx, mxy, myy, 1, nb);
    f.fin.inv = q.norm_scale * (double)std::max(1, nbias);
    return launch_finish(c, f);
}

// Every other window up to 16384 samples: the LDS-resident transform (kernels_generic.hpp), spectra of x, then the sums
// of y against them
static int welch_mean_run(ds_ctx* c, const WelchCall& q) {
    const int n_cx = q.n_cx, n_cy = q.n_cy, n_frames = q.n_frames, W = q.W;
    CHK(check_fft_len(c, W, "welch window length"));
    const float2* tw;
    CHK(get_twiddles(c, W, &tw));
    const int nb = W / 2 + 1;
    WelchPlan pl = plan_welch(n_frames, q.auto_only() ? n_cx : (n_cy + 1) / 2);
    const bool need_xs = !q.auto_only();
    float *pxx, *pyy = nullptr;
    float2 *xs = nullptr, *pxy = nullptr;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        pxx = cv.take<float>((size_t)pl.n_chunks * n_cx * nb);
        if (need_xs) {
            xs = cv.take<float2>((size_t)n_cx * n_frames * nb);
            pxy = cv.take<float2>((size_t)pl.n_chunks * n_cy * nb);
            pyy = cv.take<float>((size_t)pl.n_chunks * n_cy * nb);
        }
    }));
    {
        XspecArgs a{q.x, q.n_samples, q.ldx, n_cx, W, q.hop, n_frames, q.detrend, pl.fpc, q.window, tw, xs, pxx};
        dim3 grid(pl.n_chunks, n_cx);
        DISPATCH_N(W, CHK(launch(c, "welch_xspec", k_xspec<NN>, grid, Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, a)));
    }
    if (need_xs) {
        YaccArgs a{q.y, q.n_samples, q.ldy, n_cy, n_cx, W, q.hop, n_frames, q.detrend, pl.fpc, q.window, tw, xs, pxy, pyy};
        dim3 grid(pl.n_chunks, (n_cy + 1) / 2);
        DISPATCH_N(W, CHK(launch(c, "welch_yacc", k_yacc<NN>, grid, Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, a)));
    }
    return launch_finish(c, welch_fin(q, pxx, pxy, pyy, pl.n_chunks, nb));
}

// Frames the kernels have to visit: a frame that starts at or past the end of the signal is all
// zeros (include/dsptoolbox_amd.h: "zero padded") and adds nothing to any sum, so the pair loops
// stop at the last pair that still overlaps the signal -- no loader ever forms an address from a
// start beyond the data.  The normalisation keeps the caller's frame count.
static int frames_to_visit(int64_t n_samples, int hop, int n_frames) {
    const int64_t pairs = (n_samples + 2 * (int64_t)hop - 1) / (2 * (int64_t)hop);
    return (int)std::min<int64_t>(n_frames, 2 * pairs);
}

// nfft 4096: register-resident radix-16 FFT path (kernels_welch4096.hpp); three workgroups per CU at 50 % overlap
// (kernels_welch4096w.hpp), two otherwise
static int welch4096_run(ds_ctx* c, const WelchCall& q) {
    namespace w4 = welch4096;
    CHK(ensure_table(c, &c->w4_tables, w4::host_tables));
    const bool auto_only = q.auto_only();
    const int n_cx = q.n_cx, n_cy = q.n_cy, n_out = q.n_out();
    const int nf = frames_to_visit(q.n_samples, q.hop, q.n_frames);
    const bool half = q.hop == 2048;
    const bool three = half && !c->cfg.w4_two_per_cu && w4::fits3(q.n_samples, nf);
    w4::Plan pl = three ? w4::plan3(nf, n_out, c->cfg.welch_chunks) : w4::plan(nf, n_out, c->cfg.welch_chunks);
    float2 *xs = nullptr, *pxy = nullptr;
    float *px = nullptr, *psx = nullptr, *pyy;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        if (!auto_only) {
            xs = cv.take<float2>((size_t)n_cx * pl.n_pairs * w4::N);
            px = cv.take<float>((size_t)n_cx * pl.n_pairs * w4::NB);
            psx = cv.take<float>((size_t)pl.n_chunks * n_cx * w4::NB);
            pxy = cv.take<float2>((size_t)pl.n_chunks * n_cy * w4::NB);
        }
        pyy = cv.take<float>((size_t)pl.n_chunks * n_out * w4::NB);
    }));
    w4::Args ax{q.x, q.n_samples, q.ldx, auto_only ? n_cx : 1, q.hop, nf, pl.n_pairs, q.detrend, pl.n_chunks, pl.ppc, q.window,
                c->w4_tables, xs, px, pxy, pyy, psx};
    if (auto_only) {
        if (three) {
            w4::place_remainder(ax, n_cx);
            CHK(launch(c, "welch4096_main@3", w4::k_y3<true>, dim3(pl.n_chunks * n_cx), w4::NT, w4::LDS3_BYTES, ax));
        } else {
            auto ky = half ? w4::k_y<true, true> : w4::k_y<false, true>;
            CHK(launch(c, "welch4096_main@2", ky, dim3(pl.n_chunks * n_cx), w4::NT, w4::LDS_BYTES_2, ax));
        }
    } else {
        ax.n_cx = n_cx;
        w4::Args ay = y_args(ax, q);
        if (three) {
            w4::place_remainder(ay, n_cy);
            CHK(launch(c, "welch4096_x", w4::k_x3, dim3(pl.n_pairs * n_cx), w4::NT, w4::LDS3_BYTES, ax));
            if (n_cx > 1) CHK(launch(c, "welch4096_pxsum", w4::k_px_sum, dim3(pl.n_chunks, n_cx), 256, 0, ay));
            CHK(launch(c, "welch4096_main@3", w4::k_y3<false>, dim3(pl.n_chunks * n_cy), w4::NT, w4::LDS3_BYTES, ay));
        } else {
            auto kx = half ? w4::k_x<true> : w4::k_x<false>;
            auto ky = half ? w4::k_y<true> : w4::k_y<false>;
            CHK(launch(c, "welch4096_x", kx, dim3(pl.n_pairs, n_cx), w4::NT, w4::LDS_BYTES, ax));
            if (n_cx > 1) CHK(launch(c, "welch4096_pxsum", w4::k_px_sum, dim3(pl.n_chunks, n_cx), 256, 0, ay));
            CHK(launch(c, "welch4096_main@2", ky, dim3(pl.n_chunks * n_cy), w4::NT, w4::LDS_BYTES_2, ay));
        }
    }
    return launch_finish(c, welch_fin(q, auto_only ? pyy : psx, pxy, auto_only ? nullptr : pyy, pl.n_chunks, w4::NB));
}

// window 2048 at 50 % overlap: two 2048-point pair transforms per pass of the 4096-point register machine
// (kernels_welch2048h.hpp)
static bool welch2048h_applies(const ds_ctx* c, const WelchCall& q) {
    return q.W == 2048 && q.hop == 1024 && q.average == DS_AVG_MEAN && !c->cfg.welch_generic && !c->cfg.w2048_wave &&
           welch2048h::fits(q.n_samples, q.n_frames);
}
static int welch2048h_run(ds_ctx* c, const WelchCall& q) {
    namespace wh = welch2048h;
    namespace w4 = welch4096;
    const bool auto_only = q.auto_only();
    CHK(ensure_table(c, &c->w4_tables, w4::host_tables));
    const int n_cx = q.n_cx, n_cy = q.n_cy, n_out = q.n_out();
    const int nf = frames_to_visit(q.n_samples, wh::HOP, q.n_frames);
    wh::Plan pl = wh::plan(nf, n_out, auto_only ? 0 : n_cx, c->cfg.welch_chunks);
    float2 *xs, *pxy;
    float *px, *psx, *pyy;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        xs = auto_only ? nullptr : cv.take<float2>((size_t)n_cx * pl.n_passes * wh::PASS);
        px = auto_only ? nullptr : cv.take<float>((size_t)n_cx * pl.n_passes * wh::NBW);
        psx = auto_only ? nullptr : cv.take<float>((size_t)pl.n_chunks * n_cx * wh::NBW);
        pxy = auto_only ? nullptr : cv.take<float2>((size_t)pl.n_chunks * n_cy * wh::NBW);
        pyy = cv.take<float>((size_t)pl.n_chunks * n_out * wh::NBW);
    }));
    // (Args::n_pairs counts passes of four frames here)
    w4::Args ax{q.x, q.n_samples, q.ldx, 1, wh::HOP, nf, pl.n_passes, q.detrend, pl.n_chunks, 0, q.window, c->w4_tables, xs, px,
                pxy, pyy, psx};
    ax.n_cx = n_cx;
    if (auto_only) {
        ax.n_ch = n_cx;
        w4::place_remainder(ax, n_cx);
        CHK(launch(c, "welch2048_main@4k", wh::k_y2h<true>, dim3(pl.n_chunks * n_cx), w4::NT, wh::LDS_BYTES, ax));
        return launch_finish(c, welch_fin(q, pyy, nullptr, nullptr, pl.n_chunks, wh::NBW));
    }
    w4::Args ay = y_args(ax, q);
    w4::place_remainder(ay, n_cy);
    CHK(launch(c, "welch2048_x", wh::k_x2h, dim3(pl.n_passes * n_cx), w4::NT, wh::LDS_BYTES, ax));
    if (n_cx > 1) CHK(launch(c, "welch2048_pxsum", wh::k_px_sum, dim3(pl.n_chunks, n_cx), 256, 0, ay));
    CHK(launch(c, "welch2048_main@4k", wh::k_y2h<false>, dim3(pl.n_chunks * n_cy), w4::NT, wh::LDS_BYTES, ay));
    return launch_finish(c, welch_fin(q, psx, pxy, pyy, pl.n_chunks, wh::NBW));
}

// window 8192: two 4096-point register transforms per frame pair (kernels_welch8192.hpp)
static int welch8192_run(ds_ctx* c, const WelchCall& q) {
    namespace w8 = welch8k;
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    CHK(ensure_table(c, &c->deconv8k_tables, deconv8k::host_tables));
    const bool auto_only = q.auto_only();
    const int n_cx = q.n_cx, n_cy = q.n_cy, n_out = q.n_out();
    const int nf = frames_to_visit(q.n_samples, q.hop, q.n_frames);
    w8::Plan pl = w8::plan(nf, n_out, auto_only ? 1 : n_cx);
    float2 *xs = nullptr, *pxy = nullptr;
    float *px = nullptr, *psx = nullptr, *pyy;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        if (!auto_only) {
            xs = cv.take<float2>((size_t)n_cx * pl.n_pairs * w8::N);
            px = cv.take<float>((size_t)n_cx * pl.n_pairs * w8::NB);
            psx = cv.take<float>((size_t)pl.n_chunks * n_cx * w8::NB);
            pxy = cv.take<float2>((size_t)pl.n_chunks * n_cy * w8::NB);
        }
        pyy = cv.take<float>((size_t)pl.n_chunks * n_out * w8::NB);
    }));
    const bool half = q.hop == 4096;
    w8::Args ax{q.x, q.n_samples, q.ldx, n_cx, q.hop, nf, pl.n_pairs, q.detrend, pl.n_chunks, q.window,
                c->w4_tables, c->deconv8k_tables, (float4*)xs, px, pxy, pyy, psx, auto_only ? 0 : n_cx};
    // window in LDS + one exchange buffer per group (0.226 ms; the global-window / two-buffer
    // variant measured 0.280 ms and spilled: removed)
    if (auto_only) {
        auto ky = half ? w8::k_y<true, true, true> : w8::k_y<false, true, true>;
        CHK(launch(c, "welch8192_main", ky, dim3(pl.n_chunks * n_cx), w8::NTB, w8::LDS_BYTES_WINLDS, ax));
    } else {
        auto kx = half ? w8::k_x<true> : w8::k_x<false>;
        CHK(launch(c, "welch8192_x", kx, dim3(pl.n_pairs, n_cx), w8::NTB, w8::LDS_BYTES, ax));
        if (n_cx > 1) CHK(launch(c, "welch8192_pxsum", w8::k_px_sum, dim3(pl.n_chunks, n_cx), 256, 0, ax));
        auto ky = half ? w8::k_y<true, true> : w8::k_y<false, true>;
        CHK(launch(c, "welch8192_main", ky, dim3(pl.n_chunks * n_cy), w8::NTB, w8::LDS_BYTES_WINLDS, y_args(ax, q)));
    }
    return launch_finish(c, welch_fin(q, auto_only ? pyy : psx, pxy, auto_only ? nullptr : pyy, pl.n_chunks, w8::NB));
}

// window 16384: four 4096-point register transforms per frame pair, two per slot of 256 threads
// (kernels_welch16384.hpp)
static int welch16384_run(ds_ctx* c, const WelchCall& q) {
    namespace w16 = welch16k;
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    CHK(ensure_table(c, &c->fir16k_tables, fir16k::host_tables));
    const bool auto_only = q.auto_only();
    const int n_cx = q.n_cx, n_cy = q.n_cy, n_out = q.n_out();
    const int nf = frames_to_visit(q.n_samples, q.hop, q.n_frames);
    w16::Plan pl = w16::plan(nf, n_out, auto_only ? 1 : n_cx);
    float2 *xs = nullptr, *pxy = nullptr, *tu = nullptr;
    float *pxu = nullptr, *psx = nullptr, *pyy, *pu;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        if (!auto_only) {
            xs = cv.take<float2>((size_t)n_cx * pl.n_pairs * w16::N);
            pxu = cv.take<float>((size_t)n_cx * pl.n_pairs * w16::N);
            psx = cv.take<float>((size_t)pl.n_chunks * n_cx * w16::NB);
            pxy = cv.take<float2>((size_t)pl.n_chunks * n_cy * w16::NB);
        }
        pyy = cv.take<float>((size_t)pl.n_chunks * n_out * w16::NB);
        if (!auto_only) tu = cv.take<float2>((size_t)pl.n_chunks * n_cy * w16::N);
        pu = cv.take<float>((size_t)pl.n_chunks * n_out * w16::N);
    }));
    w16::Args ax{q.x, q.n_samples, q.ldx, n_cx, q.hop, nf, pl.n_pairs, q.detrend, pl.n_chunks, q.window,
                 c->w4_tables, c->fir16k_tables, (float4*)xs, pxu, pxy, pyy, psx, auto_only ? 1 : n_cx, tu, pu};
    if (auto_only) {
        CHK(launch(c, "welch16384_main", w16::k_y<true>, dim3(pl.n_chunks * n_cx, 1, 4), w16::NTB, w16::LDS_BYTES, ax));
        CHK(launch(c, "welch16384_fold", w16::k_fold<true>, dim3((w16::NB + 255) / 256, pl.n_chunks * n_cx), 256, 0, ax));
    } else {
        CHK(launch(c, "welch16384_x", w16::k_x, dim3(pl.n_pairs, n_cx, 4), w16::NTB, w16::LDS_BYTES, ax));
        CHK(launch(c, "welch16384_pxsum", w16::k_px_sum, dim3((w16::NB + 255) / 256, pl.n_chunks, n_cx), 256, 0, ax));
        const w16::Args ay = y_args(ax, q);
        CHK(launch(c, "welch16384_main", w16::k_y<false>, dim3(pl.n_chunks * n_cy, 1, 4), w16::NTB, w16::LDS_BYTES, ay));
        CHK(launch(c, "welch16384_fold", w16::k_fold<false>, dim3((w16::NB + 255) / 256, pl.n_chunks * n_cy), 256, 0, ay));
    }
    return launch_finish(c, welch_fin(q, auto_only ? pyy : psx, pxy, auto_only ? nullptr : pyy, pl.n_chunks, w16::NB));
}

// Windows of 2^15 ... 2^18 samples: decimation in frequency into R = W / 4096 class sequences (k_dif), the headline
// kernel's loop on them (k_xc / k_yc), fold across the classes, finish (kernels_welch_long.hpp).
static bool welch_long_applies(const ds_ctx* c, const WelchCall& q) {
    const int W = q.W, n_ch_total = q.n_cx + q.nyc();
    if (c->cfg.welch_generic || q.average != DS_AVG_MEAN || !welchl::classes_of(W) || W < c->cfg.welch_long_min) return false;
    if (!welchl::buf_fits(q.n_samples, q.n_frames, q.hop, W)) return false;
    // the class sequences: one complex value per sample of every frame pair (8 bytes per sample at 50 % overlap)
    const int64_t pairs = ((int64_t)frames_to_visit(q.n_samples, q.hop, q.n_frames) + 1) / 2;
    // launch grids: k_dif puts the frame pairs on grid.y and the channels on grid.z, k_fold (chunk, channel) units on
    // grid.y (chunks <= max(768 / R, pairs / 64), kernels_welch_long.hpp plan()); shapes beyond 65535 there (99 %
    // overlap on 2^25 samples, ...) fall through to the routes behind this one
    const int64_t chunks_max = std::max<int64_t>(768 / welchl::classes_of(W) + 1, (pairs + 63) / 64);
    if (pairs > 65535 || n_ch_total > 65535 || chunks_max * n_ch_total > 65535) return false;
    return (int64_t)n_ch_total * pairs * W * 8 <= ((int64_t)16 << 30);
}
static int welch_long_run(ds_ctx* c, const WelchCall& q) {
    namespace wl = welchl;
    const bool auto_only = q.auto_only();
    const int n_cx = q.n_cx, n_cy = q.n_cy, W = q.W;
    const int R = wl::classes_of(W);
    int lgR;
    const float2* twl;
    CHK(long_tables(c, R, &lgR, &twl));
    const int nf = frames_to_visit(q.n_samples, q.hop, q.n_frames), nb = W / 2 + 1;
    const int n_out = q.n_out();
    wl::Plan pl = wl::plan(nf, n_out, R);
    const size_t seq = (size_t)pl.n_pairs * W;  // complex values per channel
    float2 *bx, *by, *xs, *pxy, *tu;
    float *pxu, *psx, *pyy, *pu;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        bx = cv.take<float2>(seq * n_cx);
        by = auto_only ? nullptr : cv.take<float2>(seq * n_cy);
        xs = auto_only ? nullptr : cv.take<float2>(seq * n_cx);
        pxu = auto_only ? nullptr : cv.take<float>(seq * n_cx);
        psx = auto_only ? nullptr : cv.take<float>((size_t)pl.n_chunks * n_cx * nb);
        pxy = auto_only ? nullptr : cv.take<float2>((size_t)pl.n_chunks * n_cy * nb);
        tu = auto_only ? nullptr : cv.take<float2>((size_t)pl.n_chunks * n_cy * W);
        pyy = cv.take<float>((size_t)pl.n_chunks * n_out * nb);
        pu = cv.take<float>((size_t)pl.n_chunks * n_out * W);
    }));
    wl::Args ax{q.x, q.n_samples, q.ldx, n_cx, q.hop, nf, pl.n_pairs, q.detrend, pl.n_chunks, R, lgR, q.window, c->w4_tables, twl,
                bx, (float4*)xs, pxu, pxy, pyy, psx, n_cx, tu, pu};
    auto dif = [&](const wl::Args& a, int n_ch) {
        const dim3 grid(wl::M / wl::NT, pl.n_pairs, n_ch);
        return dispatch<4, 8, 16, 32, 64>(R, [&](auto r) { return launch(c, "welch_long_dif", wl::k_dif<r.value>, grid, wl::NT, 0, a); });
    };
    CHK(dif(ax, n_cx));
    const dim3 fold_grid((nb + 255) / 256, pl.n_chunks * n_out);
    if (auto_only) {
        CHK(launch(c, "welch_long_main", wl::k_yc<true>, dim3((unsigned)(pl.n_chunks * n_cx * R)), wl::NT, wl::LDS_BYTES, ax));
        CHK(launch(c, "welch_long_fold", wl::k_fold<true>, fold_grid, 256, 0, ax));
        return launch_finish(c, welch_fin(q, pyy, nullptr, nullptr, pl.n_chunks, nb));
    }
    CHK(launch(c, "welch_long_x", wl::k_xc, dim3((unsigned)(pl.n_pairs * R * n_cx)), wl::NT, wl::LDS_BYTES, ax));
    CHK(launch(c, "welch_long_pxsum", wl::k_px_sum, dim3((nb + 255) / 256, pl.n_chunks, n_cx), 256, 0, ax));
    wl::Args ay = y_args(ax, q);
    ay.b = by;
    CHK(dif(ay, n_cy));
    if (c->cfg.welch_long_3percu)
        CHK(launch(c, "welch_long_main@jit", wl::k_yc<false, true>, dim3((unsigned)(pl.n_chunks * n_cy * R)), wl::NT, wl::LDS_BYTES, ay));
    else
        CHK(launch(c, "welch_long_main", wl::k_yc<false>, dim3((unsigned)(pl.n_chunks * n_cy * R)), wl::NT, wl::LDS_BYTES, ay));
    CHK(launch(c, "welch_long_fold", wl::k_fold<false>, fold_grid, 256, 0, ay));
    return launch_finish(c, welch_fin(q, psx, pxy, pyy, pl.n_chunks, nb));
}

// windows of 256 / 512 / 1024 / 2048 samples (1024 = the reference's default): wave-level register transforms
// (kernels_welch1024.hpp).  W < NN (windows of 128 / 64 / 32 samples on the 256-point kernels): the frames are
// transformed zero-padded to NN points and every (NN / W)-th bin is kept (removing a frame's mean still only clears
// bin 0 of the kept bins)
template <int NN>
static int welch_wave_run(ds_ctx* c, const WelchCall& q) {
    namespace w1 = welch1k;
    using G = w1::WG<NN>;
    const float2* tab;
    CHK(wave_tables<NN>(c, &tab));
    const bool auto_only = q.auto_only();
    const int n_cx = q.n_cx, n_cy = q.n_cy, n_out = q.n_out();
    const int decim = NN / q.W;
    const int nf = frames_to_visit(q.n_samples, q.hop, q.n_frames);
    w1::Plan pl = w1::plan<NN>(nf, n_out, auto_only ? 1 : n_cx, c->cfg.welch1k_chunks);
    float *wz, *px = nullptr, *psx = nullptr, *pyy;
    float2 *xs = nullptr, *pxy = nullptr;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        wz = decim > 1 ? cv.take<float>(NN) : nullptr;
        if (!auto_only) {
            xs = cv.take<float2>((size_t)n_cx * pl.n_pairs * NN);
            px = cv.take<float>((size_t)n_cx * pl.n_pairs * G::NB);
            psx = cv.take<float>((size_t)pl.n_chunks * n_cx * G::NB);
            pxy = cv.take<float2>((size_t)pl.n_chunks * n_cy * G::NB);
        }
        pyy = cv.take<float>((size_t)pl.n_chunks * n_out * G::NB);
    }));
    const float* window = q.window;
    if (decim > 1) {  // the window, zero-padded to the transform length
        HIPCHK(c, hipMemsetAsync(wz, 0, sizeof(float) * NN, c->stream));
        HIPCHK(c, hipMemcpyAsync(wz, window, sizeof(float) * (NN / decim), hipMemcpyDeviceToDevice, c->stream));
        window = wz;
    }
    const bool half = q.hop == NN / 2;
    w1::Args ax{q.x, q.n_samples, q.ldx, n_cx, q.hop, nf, pl.n_pairs, q.detrend, pl.n_chunks, pl.ppc, window,
                tab, (float4*)xs, px, pxy, pyy, psx, auto_only ? 1 : n_cx};
    const int n_grp = (n_out + G::TPB - 1) / G::TPB;
    if (auto_only) {
        auto ky = half ? w1::k_y<NN, true, true> : w1::k_y<NN, false, true>;
        CHK(launch(c, "welch1024_main", ky, dim3(pl.n_chunks * n_grp), w1::NTB, G::LDS_BYTES, ax));
    } else {
        auto kx = half ? w1::k_x<NN, true> : w1::k_x<NN, false>;
        auto ky = half ? w1::k_y<NN, true> : w1::k_y<NN, false>;
        CHK(launch(c, "welch1024_x", kx, dim3((pl.n_pairs + G::TPB - 1) / G::TPB, n_cx), w1::NTB, G::LDS_BYTES, ax));
        if (n_cx > 1) CHK(launch(c, "welch1024_pxsum", w1::k_px_sum<NN>, dim3(pl.n_chunks, n_cx), 256, 0, ax));
        CHK(launch(c, "welch1024_main", ky, dim3(pl.n_chunks * n_grp), w1::NTB, G::LDS_BYTES, y_args(ax, q)));
    }
    WelchFinArgs f = welch_fin(q, auto_only ? pyy : psx, pxy, auto_only ? nullptr : pyy, pl.n_chunks, NN / decim / 2 + 1);
    f.in_nb = G::NB;
    f.in_step = decim;
    return launch_finish(c, f);
}

// What every Welch entry checks of its call, once, before anything is staged or launched
static int welch_check(ds_ctx* c, const WelchCall& q) {
    if (!c || !q.x || !q.window) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if ((q.kind != PSD && !q.out_c) || (q.kind != CSD && !q.out_r)) return fail(c, DS_ERR_ARG, q.who, "null output");
    if (q.average != DS_AVG_MEAN && q.average != DS_AVG_MEDIAN)
        return fail(c, DS_ERR_ARG, q.who, "average must be mean (0) or median (1)");
    if (!q.auto_only() && !q.y) return fail(c, DS_ERR_ARG, q.who, "null output-signal pointer");
    if (q.n_cx <= 0 || q.n_samples <= 0 || q.hop <= 0 || q.hop > q.W || q.n_frames <= 0 || q.ldx < q.n_samples)
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (!q.auto_only() && (q.n_cy <= 0 || q.ldy < q.n_samples || !(q.n_cx == 1 || q.n_cx == q.n_cy)))
        return fail(c, DS_ERR_ARG, q.who, "input must have 1 channel or as many as the output");
    if (q.kind == TF && (q.mode < DS_TF_H1 || q.mode > DS_TF_H3))
        return fail(c, DS_ERR_ARG, q.who, "unsupported transfer function type");
    return DS_OK;
}

using WelchRunner = int (*)(ds_ctx*, const WelchCall&);
// The kernel family of a checked call: the register kernels of its window where they apply; behind them the four-step
// transforms for windows beyond the LDS-resident FFT and the generic LDS kernels (medians, means) for the others.
static WelchRunner welch_route(const ds_ctx* c, const WelchCall& q) {
    const int W = q.W;
    const WelchRunner rest = q.big() ? welch_big_run : (q.average == DS_AVG_MEDIAN ? welch_median_run : welch_mean_run);
    if (q.average != DS_AVG_MEAN) return rest;
    const bool generic = c->cfg.welch_generic;
    // (DSPTOOLBOX_AMD_WELCH_GENERIC keeps transfer functions with 4096-sample windows on the register kernels)
    if (W == 4096 && !c->cfg.no_welch4096 && (q.kind == TF || !generic)) return welch4096_run;
    if (welch_long_applies(c, q)) return welch_long_run;
    if (generic) return rest;
    if (W == 16384 && welch16k::buf_fits(q.n_samples, q.n_frames, q.hop)) return welch16384_run;
    if (W == 8192 && welch8k::buf_fits(q.n_samples, q.n_frames, q.hop)) return welch8192_run;
    if (welch2048h_applies(c, q)) return welch2048h_run;
    // the wave kernels: the accumulated channels (y; auto spectra: x) must fit their buffer descriptors
    if (W > 2048 || W < 32 || !welch1k::buf_fits(q.n_samples, q.n_out(), q.auto_only() ? q.ldx : q.ldy)) return rest;
    switch (W) {
        case 2048: return welch_wave_run<2048>;
        case 1024: return welch_wave_run<1024>;
        case 512: return welch_wave_run<512>;
        case 256: case 128: case 64: case 32: return welch_wave_run<256>;
        default: return rest;
    }
}

// The device entry points: check, choose the route, run it.
static int welch_dev(ds_ctx* c, const WelchCall& q) {
    CHK(welch_check(c, q));
    return welch_route(c, q)(c, q);
}

extern "C" int ds_welch_tf_dev(ds_ctx* c, const float* x, int n_cx, int64_t ldx, const float* y,
                               int n_cy, int64_t ldy, int64_t n_samples, int W, int hop, int n_frames,
                               const float* window, int detrend, int average, int mode, int amp_sqrt,
                               double norm_scale, double factor, int halve_edges, ds_c32* tf,
                               float* coh) {
    return welch_dev(c, {"ds_welch_tf_dev", TF, x, n_cx, ldx, y, n_cy, ldy, n_samples, W, hop, n_frames, window, detrend,
                         average, mode, amp_sqrt, norm_scale, factor, halve_edges, (float2*)tf, coh});
}
extern "C" int ds_welch_psd_dev(ds_ctx* c, const float* x, int n_cx, int64_t ldx, int64_t n_samples,
                                int W, int hop, int n_frames, const float* window, int detrend,
                                int average, int amp_sqrt, double norm_scale, double factor,
                                int halve_edges, float* psd) {
    return welch_dev(c, {"ds_welch_psd_dev", PSD, x, n_cx, ldx, nullptr, 0, 0, n_samples, W, hop, n_frames, window, detrend,
                         average, 0, amp_sqrt, norm_scale, factor, halve_edges, nullptr, psd});
}
// ---- Welch in float64 end to end (kernels_welch_f64.hpp) ---------------------------------------------------------
// The three entries below take host arrays in the reference's own layouts, (samples, channels) float64, and answer in
// complex128 / float64.  Each fills one X64Call, has x64_check judge it (and adds the limits only it has), carves its pieces
// out of c->io, fills the tables, has x64_frames upload and transform each signal, launches its own mean or median kernel
// on x64_finish's FinishPar, downloads and synchronises once.  `who` is the entry's name in its error messages.
static const int kMaxX64Window = 262144;
static const int64_t kMaxX64PlanarSamples = (int64_t)0x7fffffff * 32;  // w64::k_planar: 32 samples per workgroup of grid.x

// ds_welch_tf_x64: out (tf) and coh of y against x, n_cx = 1 or n_cy.  ds_welch_spec_x64: auto spectra of x or, with y, the
// cross spectra conj(X_i) Y_i (n_cy = 0 or n_cx); ds_csm_x64: the matrix of x (y null).  These two: coh null, mode 0.
struct X64Call {
    const char* who;
    const double* x; int n_cx; const double* y; int n_cy; int64_t n_samples; int W, hop, n_frames;
    const double* window; int detrend, average, mode, amp_sqrt; double norm_scale, factor; int halve_edges;
    double *out, *coh;
    int nb() const { return W / 2 + 1; }
    bool median() const { return average == DS_AVG_MEDIAN; }
};
// What all three refuse.  n_spectra_x / n_spectra_y: the channels of x and y whose frame spectra the call holds: 2 GiB at most
static int x64_check(ds_ctx* c, const X64Call& q, int n_spectra_x, int n_spectra_y) {
    if (!c || !q.x || !q.window || !q.out) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.average != DS_AVG_MEAN && q.average != DS_AVG_MEDIAN)
        return fail(c, DS_ERR_ARG, q.who, "average must be mean (0) or median (1)");
    if (q.median() && q.n_frames > 4096)
        return fail(c, DS_ERR_UNSUP, q.who, "median averaging over more than 4096 frames (use the fp32 entry point)");
    if (n_spectra_x <= 0 || n_spectra_y < 0 || q.n_samples <= 0 || q.hop <= 0 || q.hop > q.W || q.n_frames <= 0)
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (!is_pow2(q.W) || q.W < 8 || q.W > kMaxX64Window)
        return fail(c, DS_ERR_UNSUP, q.who, "window length must be a power of two in [8, 262144]");
    if (((size_t)n_spectra_x + (size_t)n_spectra_y) * q.n_frames * q.nb() * sizeof(double2) > ((size_t)2 << 30))
        return fail(c, DS_ERR_UNSUP, q.who, "problem too large for the float64 route (use the fp32 entry point)");
    return DS_OK;
}
// the finish of the mean over the frames, or of the median with the reference's bias correction
static FinishPar x64_finish(const X64Call& q, int nb) {
    const int nbias = (q.n_frames & 1) ? q.n_frames : q.n_frames - 1;
    return {q.median() ? q.norm_scale * (double)std::max(1, nbias) : q.norm_scale / (double)q.n_frames, q.factor, q.halve_edges,
            q.amp_sqrt, nb};
}

// planar[n_ch][n_samples] of the device-resident (samples, channels) array dsig
static int x64_planar(ds_ctx* c, const double* dsig, int64_t n_samples, int n_ch, double* planar) {
    if (n_samples > kMaxX64PlanarSamples)
        return fail(c, DS_ERR_UNSUP, "float64 Welch route: signal too long for the long-window kernels");
    hipLaunchKernelGGL(w64::k_planar, dim3((unsigned)((n_samples + 31) / 32), (unsigned)((n_ch + 31) / 32)), dim3(256), 0, c->stream,
                       dsig, n_samples, n_ch, planar);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

// the float64 window and twiddle tables of the x64 entries: carved by take_x64_tables, filled by x64_tables
struct X64Tables {
    double* dw;
    double2* tw;
};
static X64Tables take_x64_tables(Carver& cv, int W) { return {cv.take<double>(W), cv.take<double2>(W / 2)}; }
static int x64_tables(ds_ctx* c, const X64Tables& t, const double* window, int W) {
    HIPCHK(c, hipMemcpyAsync(t.dw, window, (size_t)W * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(w64::k_twiddles, dim3((W / 2 + 255) / 256), dim3(256), 0, c->stream, t.tw, W / 2);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

// float64 frame spectra of a device-resident (samples, channels) float64 array: W <= 16384 one workgroup per
// (frame, channel); 2^15 ... 2^18 one per (frame, class, channel) + the split (class spectra in the workspace)
static int x64_launch_frames(ds_ctx* c, const X64Call& q, const X64Tables& t, const double* dsig, int n_ch, double2* spec) {
    const int W = q.W, n_frames = q.n_frames;
    const int64_t n_samples = q.n_samples;
    int lg = 0;
    while ((1 << lg) < W) ++lg;
    w64::FrameArgs fa{dsig, n_samples, n_ch, W, lg, q.hop, n_frames, q.detrend, t.dw, t.tw, spec, n_ch, 1};
    if (W <= 16384) {
        // four channels or more: read a planar copy (one 8-byte value per 32-byte sector otherwise)
        if (n_ch >= 4 && n_samples <= kMaxX64PlanarSamples) {
            CHK(reserve(c, &c->ws, &c->ws_bytes, sizeof(double) * (size_t)n_ch * n_samples));
            double* planar = (double*)c->ws;
            CHK(x64_planar(c, dsig, n_samples, n_ch, planar));
            fa.sig = planar;
            fa.s_stride = 1;
            fa.c_stride = n_samples;
        }
        const bool packed = W > 8192;  // the real frame as a W/2-point complex sequence: 128 KB of LDS either way
        const size_t lds = (size_t)(packed ? W / 2 : W) * 16 + 256 * 8;
        auto frames = packed ? w64::k_frames<true> : w64::k_frames<false>;
        return launch(c, "welch_f64_frames", frames, dim3(n_frames, n_ch), 256, lds, fa);
    }
    const int rc = (W / 2) / w64::LONG_M;
    int lg_rc = 0;
    while ((1 << lg_rc) < rc) ++lg_rc;
    if ((int64_t)n_frames * rc > 0x7fffffff || n_ch > 65535 || n_frames > 65535)
        return fail(c, DS_ERR_UNSUP, "float64 Welch route: too many frames / channels for the long-window kernels");
    double2* zc;
    double* planar;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        zc = cv.take<double2>((size_t)n_ch * n_frames * (W / 2));
        planar = cv.take<double>((size_t)n_ch * n_samples);
    }));
    CHK(x64_planar(c, dsig, n_samples, n_ch, planar));  // (these kernels read nothing else: an over-long signal ends here)
    w64::LongArgs la{fa, rc, lg_rc, zc, planar};
    CHK(launch(c, "welch_f64_frames@long", w64::k_frames_cls, dim3((unsigned)(n_frames * rc), n_ch), 256,
               (size_t)w64::LONG_M * 16 + 256 * 8, la));
    return launch(c, "welch_f64_split", w64::k_split, dim3((W / 2 + 1 + 255) / 256, n_frames, n_ch), 256, 0, la);
}
// the same of a host array sig: uploaded to dsig first
static int x64_frames(ds_ctx* c, const X64Call& q, const X64Tables& t, const double* sig, double* dsig, int n_ch, double2* spec) {
    HIPCHK(c, hipMemcpyAsync(dsig, sig, (size_t)q.n_samples * n_ch * 8, hipMemcpyHostToDevice, c->stream));
    return x64_launch_frames(c, q, t, dsig, n_ch, spec);
}

extern "C" int ds_welch_tf_x64(ds_ctx* c, const double* x, int n_cx, const double* y, int n_cy,
                               int64_t n_samples, int W, int hop, int n_frames, const double* window,
                               int detrend, int average, int mode, int amp_sqrt, double norm_scale,
                               double factor, int halve_edges, double* tf, double* coh) {
    const X64Call q{"ds_welch_tf_x64", x, n_cx, y, n_cy, n_samples, W, hop, n_frames, window, detrend, average, mode,
                    amp_sqrt, norm_scale, factor, halve_edges, tf, coh};
    // (its own argument errors first: beside a window or a size that is not built they stay DS_ERR_ARG)
    if (!y || !coh) return fail(c, DS_ERR_ARG, "ds_welch_tf_x64: null argument");
    if (n_cy <= 0 || (n_cx != 1 && n_cx != n_cy)) return fail(c, DS_ERR_ARG, "ds_welch_tf_x64: bad shape");
    if (mode < DS_TF_H1 || mode > DS_TF_H3) return fail(c, DS_ERR_ARG, "ds_welch_tf_x64: unsupported transfer function type");
    CHK(x64_check(c, q, n_cx, n_cy));
    HIPCHK(c, hipSetDevice(c->device));
    const int nb = q.nb();
    const size_t bout = (size_t)nb * n_cy;
    double *dx, *dy, *dcoh;
    double2 *xs, *ys, *dtf;
    X64Tables t;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        dx = cv.take<double>((size_t)n_samples * n_cx);
        dy = cv.take<double>((size_t)n_samples * n_cy);
        t = take_x64_tables(cv, W);
        xs = cv.take<double2>((size_t)n_cx * n_frames * nb);
        ys = cv.take<double2>((size_t)n_cy * n_frames * nb);
        dtf = cv.take<double2>(bout);
        dcoh = cv.take<double>(bout);
    }));
    CHK(x64_tables(c, t, window, W));
    CHK(x64_frames(c, q, t, x, dx, n_cx, xs));
    CHK(x64_frames(c, q, t, y, dy, n_cy, ys));
    w64::TfArgs ta{xs, ys, n_cx, n_cy, n_frames, mode, x64_finish(q, nb), dtf, dcoh};
    if (q.median())
        CHK(launch(c, "welch_f64_tf_median", w64::k_tf_median, dim3(nb, n_cy), 256,
                   sizeof(double) * (4 * (size_t)n_frames + 8), ta));
    else
        CHK(launch(c, "welch_f64_tf", w64::k_tf, dim3((nb + 255) / 256, n_cy), 256, 0, ta));
    HIPCHK(c, hipMemcpyAsync(tf, dtf, bout * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(coh, dcoh, bout * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DS_OK;
}

// _welch (auto spectra: y = NULL; cross spectra conj(X_i) Y_i otherwise): the route backend._welch takes for SHORT
// estimates.  out: [nb][n_ch] complex128 (auto spectra: imaginary part 0).
extern "C" int ds_welch_spec_x64(ds_ctx* c, const double* x, const double* y, int n_ch, int64_t n_samples, int W,
                                 int hop, int n_frames, const double* window, int detrend, int average, int amp_sqrt,
                                 double norm_scale, double factor, int halve_edges, double* out) {
    const X64Call q{"ds_welch_spec_x64", x, n_ch, y, y ? n_ch : 0, n_samples, W, hop, n_frames, window, detrend, average, 0,
                    amp_sqrt, norm_scale, factor, halve_edges, out, nullptr};
    CHK(x64_check(c, q, n_ch, q.n_cy));
    HIPCHK(c, hipSetDevice(c->device));
    const int nb = q.nb();
    const size_t spec = (size_t)n_ch * n_frames * nb, bout = (size_t)nb * n_ch;
    X64Tables t;
    double *dx, *dy = nullptr;
    double2 *xs, *ys = nullptr, *dout;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        t = take_x64_tables(cv, W);
        dx = cv.take<double>((size_t)n_samples * n_ch);
        xs = cv.take<double2>(spec);
        if (y) {
            dy = cv.take<double>((size_t)n_samples * n_ch);
            ys = cv.take<double2>(spec);
        }
        dout = cv.take<double2>(bout);
    }));
    CHK(x64_tables(c, t, window, W));
    CHK(x64_frames(c, q, t, x, dx, n_ch, xs));
    if (y) CHK(x64_frames(c, q, t, y, dy, n_ch, ys));
    w64::SpecArgs sa{xs, ys, n_ch, n_frames, x64_finish(q, nb), dout};
    if (q.median())
        CHK(launch(c, "welch_f64_spec_median", w64::k_spec_median, dim3(nb, n_ch), 256, sizeof(double) * (2 * (size_t)n_frames + 4), sa));
    else
        CHK(launch(c, "welch_f64_spec", w64::k_spec, dim3((nb + 255) / 256, n_ch), 256, 0, sa));
    HIPCHK(c, hipMemcpyAsync(out, dout, bout * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DS_OK;
}

// _csm_welch (up to 1024 channels; median averaging: up to 128 frames): csm [nb][n_ch][n_ch] complex128
extern "C" int ds_csm_x64(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, int W, int hop, int n_frames,
                          const double* window, int detrend, int average, int amp_sqrt, double norm_scale, double factor,
                          int halve_edges, double* csm) {
    const X64Call q{"ds_csm_x64", x, n_ch, nullptr, 0, n_samples, W, hop, n_frames, window, detrend, average, 0,
                    amp_sqrt, norm_scale, factor, halve_edges, csm, nullptr};
    CHK(x64_check(c, q, n_ch, 0));
    if (n_ch > w64::CSM_MAX_CH) return fail(c, DS_ERR_UNSUP, "ds_csm_x64: more than 1024 channels (use ds_csm)");
    if (q.median() && n_frames > w64::CSM_MEDIAN_MAX_FRAMES)
        return fail(c, DS_ERR_UNSUP, "ds_csm_x64: median averaging over more than 128 frames (use ds_csm)");
    HIPCHK(c, hipSetDevice(c->device));
    const int nb = q.nb();
    const size_t bout = (size_t)nb * n_ch * n_ch;
    X64Tables t;
    double* dx;
    double2 *xs, *dcsm;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        t = take_x64_tables(cv, W);
        dx = cv.take<double>((size_t)n_samples * n_ch);
        xs = cv.take<double2>((size_t)n_ch * n_frames * nb);
        dcsm = cv.take<double2>(bout);
    }));
    CHK(x64_tables(c, t, window, W));
    CHK(x64_frames(c, q, t, x, dx, n_ch, xs));
    w64::CsmArgs ca{xs, n_ch, n_frames, x64_finish(q, nb), dcsm};
    if (q.median()) {
        CHK(launch(c, "csm_f64_median", w64::k_csm_median, dim3(nb, w64::csm_median_tile_pairs(n_ch)), 256,
                   w64::csm_median_lds(n_ch, n_frames), ca));
    } else {
        const int tile = std::max(1, std::min(n_frames, 4096 / n_ch));  // <= 64 KB of frame values per workgroup
        // (k_csm takes `tile` as a second kernel argument, which launch() does not pass: launched and recorded by hand)
        hipLaunchKernelGGL(w64::k_csm, dim3(nb, w64::csm_pair_groups(n_ch)), dim3(256), (size_t)n_ch * tile * 16, c->stream, ca, tile);
        HIPCHK(c, hipGetLastError());
        c->routes.insert("csm_f64");
    }
    HIPCHK(c, hipMemcpyAsync(csm, dcsm, bout * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DS_OK;
}

// ---- CSM -------------------------------------------------------------------
// One call of ds_csm_dev / ds_csm_bins_dev (bins [bin_start, bin_start + bin_count)), checked by csm_check; `who`: its name
struct CsmCall {
    const char* who;
    const float* x; int n_ch; int64_t ld, n_samples; int W, hop, n_frames; const float* window; int detrend, average;
    int amp_sqrt; double norm_scale, factor; int halve_edges, bin_start, bin_count; float2* csm;
    bool big() const { return W > kMaxFft && is_pow2(W); }  // window beyond the LDS-resident FFT: four-step transforms
    bool all_bins() const { return bin_start == 0 && bin_count == W / 2 + 1; }
};
static int csm_check(ds_ctx* c, const CsmCall& q) {
    const std::string w(q.who);
    if (!c || !q.x || !q.window || !q.csm) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_ch < 1 || q.n_samples <= 0 || q.hop <= 0 || q.hop > q.W || q.n_frames <= 0 || q.ld < q.n_samples)
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (q.average != DS_AVG_MEAN && q.average != DS_AVG_MEDIAN)
        return fail(c, DS_ERR_ARG, q.who, "average must be mean (0) or median (1)");
    if (!q.big()) CHK(check_fft_len(c, q.W, (w + " window length").c_str()));
    if (q.bin_start < 0 || q.bin_count <= 0 || q.bin_start + q.bin_count > q.W / 2 + 1)
        return fail(c, DS_ERR_ARG, q.who, "bad bin range");
    if (q.average == DS_AVG_MEDIAN && !q.all_bins())
        return fail(c, DS_ERR_UNSUP, q.who, "a bin range with median averaging is not built yet");
    size_t lds = 0;
    if (q.average == DS_AVG_MEDIAN && !median_bins_per_block(2, q.n_frames, &lds))
        return fail(c, DS_ERR_UNSUP, q.who, "median averaging over more than 19 199 frames is not built yet");
    return DS_OK;
}

// spectra of every frame [c][F][nb] -> per-pair, per-bin medians
static int csm_median_run(ds_ctx* c, const CsmCall& q) {
    const int nb = q.W / 2 + 1;
    size_t lds = 0;
    const int bpb = median_bins_per_block(2, q.n_frames, &lds);
    WelchPlan pl = plan_welch(q.n_frames, q.n_ch);
    float2* xsp;
    BigScratch s;
    float* scratch;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        xsp = cv.take<float2>((size_t)q.n_ch * q.n_frames * nb);
        if (q.big()) s = take_big_scratch(cv, q.n_ch, q.n_frames, q.W);
        else scratch = cv.take<float>((size_t)pl.n_chunks * q.n_ch * nb);
    }));
    if (q.big()) {
        CHK(stft_big(c, s, window_spectra(q, q.x, q.n_ch, q.ld, xsp), 0));
    } else {
        const float2* tw;
        CHK(get_twiddles(c, q.W, &tw));
        XspecArgs ax{q.x, q.n_samples, q.ld, q.n_ch, q.W, q.hop, q.n_frames, q.detrend, pl.fpc, q.window, tw, xsp, scratch};
        DISPATCH_N(q.W, CHK(launch(c, "welch_xspec", k_xspec<NN>, dim3(pl.n_chunks, q.n_ch), Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, ax)));
    }
    const int nbias = (q.n_frames & 1) ? q.n_frames : q.n_frames - 1;
    CsmMedianArgs m{xsp, q.n_ch, q.n_frames, bpb,
                    FinishPar{q.norm_scale * (double)std::max(1, nbias), q.factor, q.halve_edges, q.amp_sqrt, nb}, q.csm};
    return launch(c, "csm_median", k_csm_median, dim3((nb + bpb - 1) / bpb, q.n_ch * (q.n_ch + 1) / 2), 256, lds, m);
}

// Round 5: the 64-microphone shape in frame chunks on two streams.  Transform and product are both streams of the
// spectrogram X (written once, read once: 4.9 x the algorithmic bytes of the step, and each kernel alone reaches
// 0.4 of the HBM roofline); with the frames cut into chunks the transform of chunk k + 1 (main stream) runs beside
// the product of chunk k (side stream), the products carrying their raw fp32 sums from chunk to chunk
// (CsmArgs::part_in / part_out: 8.5 MB per hand-over against 66 MB of spectrogram per chunk).
static int csm_chunks(const ds_ctx* c, const CsmCall& q) { return std::min(c->cfg.csm_chunks, q.n_frames / 64); }
// frame f of a chunk that starts at frame f0 is frame f0 + f of the signal: the chunk's transform reads x + f0 hop
static bool pad_ok_for_chunks(int64_t n_samples, int hop, int n_frames) {
    return (int64_t)(n_frames - 1) * hop < n_samples;  // every chunk starts inside the signal
}
static int csm_chunked_run(ds_ctx* c, const CsmCall& q) {
    const int nb = q.W / 2 + 1, n_ch = q.n_ch, n_frames = q.n_frames, hop = q.hop, K = csm_chunks(c, q);
    const size_t part_elems = (size_t)nb * n_ch * n_ch;
    float2 *X, *part;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        X = cv.take<float2>((size_t)nb * n_frames * n_ch);
        part = cv.take<float2>(part_elems);
    }));
    if (c->ev_chunk[0] == nullptr)
        for (auto& e : c->ev_chunk) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipStream_t main_stream = c->stream;
    // the side stream starts behind everything already queued on the main one (the previous call's product reads X)
    HIPCHK(c, hipEventRecord(c->ev_fork, main_stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    int rc = DS_OK;
    for (int k = 0; k < K && rc == DS_OK; ++k) {
        const int f0 = (int)((int64_t)k * n_frames / K), f1 = (int)((int64_t)(k + 1) * n_frames / K), fk = f1 - f0;
        float2* Xk = X + (size_t)nb * f0 * n_ch;  // chunk k: [nb][fk][n_ch]
        rc = ds_stft_r2c_dev(c, q.x + (int64_t)f0 * hop, q.n_samples - (int64_t)f0 * hop, n_ch, q.ld, q.W, hop, q.W, 0, fk,
                             q.window, q.detrend, 1.0f, 1.0f, 0, (ds_c32*)Xk);
        if (rc != DS_OK) break;
        HIPCHK(c, hipEventRecord(c->ev_chunk[k], main_stream));
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_chunk[k], 0));
        CsmArgs a{Xk, n_ch, fk, FinishPar{q.norm_scale / (double)n_frames, q.factor, q.halve_edges, q.amp_sqrt, nb}, q.csm, 0};
        a.part_in = k > 0 ? part : nullptr;
        a.part_out = k + 1 < K ? part : nullptr;
        c->stream = c->side;  // launch() enqueues on the context's stream
        rc = launch(c, "csm_gemm@b3", csmb3::k_csm_gemm64_b3, dim3(nb - 1), 256, 0, a);
        c->stream = main_stream;
    }
    // the main stream goes on behind the last product
    HIPCHK(c, hipEventRecord(c->ev_join, c->side));
    HIPCHK(c, hipStreamWaitEvent(main_stream, c->ev_join, 0));
    return rc;
}

// the STFT X[b][f][c] (+ the four-step scratch for long windows) in the workspace, then one of the products
static int csm_gemm_run(ds_ctx* c, const CsmCall& q) {
    const int nb = q.W / 2 + 1, n_ch = q.n_ch;
    float2* X;
    BigScratch s;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        X = cv.take<float2>((size_t)nb * q.n_frames * n_ch);
        if (q.big()) s = take_big_scratch(cv, n_ch, q.n_frames, q.W);
    }));
    if (q.big())
        CHK(stft_big(c, s, window_spectra(q, q.x, n_ch, q.ld, X), 1));
    else
        CHK(ds_stft_r2c_dev(c, q.x, q.n_samples, n_ch, q.ld, q.W, q.hop, q.W, 0, q.n_frames, q.window, q.detrend, 1.0f, 1.0f,
                            0, (ds_c32*)X));
    CsmArgs a{X, n_ch, q.n_frames, FinishPar{q.norm_scale / (double)q.n_frames, q.factor, q.halve_edges, q.amp_sqrt, nb},
              q.csm, q.bin_start};
    // matrix-core products from 8 frames on (DSPTOOLBOX_AMD_CSM_GENERIC=1: never); b3: from bf16 triples on the 16 x faster
    // bf16 matrix pipe (kernels_csm_b3.hpp; DSPTOOLBOX_AMD_CSM_F32=1 keeps the fp32 matrix instructions)
    const bool mfma = q.n_frames >= 8 && !c->cfg.csm_generic, b3 = mfma && !c->cfg.csm_f32;
    // up to 64 channels: one workgroup per bin shares the operand loads between the three tile
    // pairs (the spectra of an even-length real transform are purely real at both edge bins,
    // which the kernel relies on)
    if (n_ch <= 64 && mfma && q.all_bins() && nb >= 3) {
        if (b3 && csmb3::fits(n_ch, q.n_frames)) return launch(c, "csm_gemm@b3", csmb3::k_csm_gemm64_b3, dim3(nb - 1), 256, 0, a);
        return launch(c, "csm_gemm@f32", k_csm_gemm64, dim3(nb - 1), 256, 0, a);
    }
    if (n_ch <= 64 && b3 && !q.all_bins() && csmb3::fits(n_ch, q.n_frames))
        return launch(c, "csm_gemm@b3_range", csmb3::k_csm_gemm64_b3_range, dim3(q.bin_count), 256, 0, a);
    if (n_ch > 64 && b3 && csmb3::fits_groups(n_ch, q.n_frames)) {
        // groups of 64 channels: the diagonal blocks, then the blocks below the diagonal (two workgroups each)
        const int ng = (n_ch + 63) / 64;
        a.n_groups = ng;
        a.n_groups_bins = q.bin_count;
        CHK(launch(c, "csm_gemm@group_b3", csmb3::k_csm_group_b3, dim3(q.bin_count, ng), 256, 0, a));
        return launch(c, "csm_gemm_offdiag", csmb3::k_csm_offdiag_b3, dim3(16 * ((q.bin_count + 7) / 8), ng * (ng - 1) / 2),
                      256, 0, a);
    }
    const int nt = (n_ch + 31) / 32;
    return launch(c, "csm_gemm@generic", k_csm_gemm, dim3(q.bin_count, nt * (nt + 1) / 2), 256, 0, a);
}

using CsmRunner = int (*)(ds_ctx*, const CsmCall&);
// The runner of a checked call: medians, the frame-chunked product (DSPTOOLBOX_AMD_CSM_CHUNKS), or transform + product
static CsmRunner csm_route(const ds_ctx* c, const CsmCall& q) {
    if (q.average == DS_AVG_MEDIAN) return csm_median_run;
    if (csm_chunks(c, q) >= 2 && !q.big() && q.all_bins() && q.n_ch <= 64 && q.W / 2 + 1 >= 3 && !c->cfg.csm_generic &&
        !c->cfg.csm_f32 && csmb3::fits(q.n_ch, q.n_frames) && pad_ok_for_chunks(q.n_samples, q.hop, q.n_frames))
        return csm_chunked_run;
    return csm_gemm_run;
}
static int csm_dev(ds_ctx* c, const CsmCall& q) {
    CHK(csm_check(c, q));
    return csm_route(c, q)(c, q);
}

extern "C" int ds_csm_dev(ds_ctx* c, const float* x, int n_ch, int64_t ld, int64_t n_samples, int W,
                          int hop, int n_frames, const float* window, int detrend, int average,
                          int amp_sqrt, double norm_scale, double factor, int halve_edges, ds_c32* csm) {
    return csm_dev(c, {"ds_csm_dev", x, n_ch, ld, n_samples, W, hop, n_frames, window, detrend, average, amp_sqrt, norm_scale,
                       factor, halve_edges, 0, W / 2 + 1, (float2*)csm});
}

// bins [bin_start, bin_start + bin_count) only (csm_dev[0] = matrix of bin_start): the multi-GPU
// split of the CSM -- every rank transforms all channels and keeps its own bin range
extern "C" int ds_csm_bins_dev(ds_ctx* c, const float* x, int n_ch, int64_t ld, int64_t n_samples, int W,
                               int hop, int n_frames, const float* window, int detrend, int amp_sqrt,
                               double norm_scale, double factor, int halve_edges, int bin_start,
                               int bin_count, ds_c32* csm) {
    return csm_dev(c, {"ds_csm_bins_dev", x, n_ch, ld, n_samples, W, hop, n_frames, window, detrend, DS_AVG_MEAN, amp_sqrt,
                       norm_scale, factor, halve_edges, bin_start, bin_count, (float2*)csm});
}

static int csm_spec_check(ds_ctx* c, const void* X, const void* csm, int n_bins, int n_frames, int n_ch) {
    if (!c || !X || !csm) return fail(c, DS_ERR_ARG, "ds_csm_spec: null argument");
    if (n_bins <= 0 || n_frames <= 0 || n_ch <= 0) return fail(c, DS_ERR_ARG, "ds_csm_spec: bad shape");
    return DS_OK;
}

extern "C" int ds_csm_spec_dev(ds_ctx* c, const ds_c32* X, int n_bins, int n_frames, int n_ch,
                               int amp_sqrt, double norm_scale, double factor, int halve_edges,
                               ds_c32* csm) {
    CHK(csm_spec_check(c, X, csm, n_bins, n_frames, n_ch));
    const int nt = (n_ch + 31) / 32;
    CsmArgs a{(const float2*)X, n_ch, n_frames,
              FinishPar{norm_scale / (double)n_frames, factor, halve_edges, amp_sqrt, n_bins},
              (float2*)csm, 0};
    CHK(launch(c, "csm_gemm@generic", k_csm_gemm, dim3(n_bins, nt * (nt + 1) / 2), 256, 0, a));
    return DS_OK;
}

extern "C" int ds_csm_spec(ds_ctx* c, const ds_c32* X, int n_bins, int n_frames, int n_ch, int amp_sqrt,
                           double norm_scale, double factor, int halve_edges, ds_c32* csm) {
    CHK(csm_spec_check(c, X, csm, n_bins, n_frames, n_ch));
    const size_t nx = (size_t)n_bins * n_frames * n_ch, no = (size_t)n_bins * n_ch * n_ch;
    return staged(c, {{8, nx, X, nullptr}, {8, no, nullptr, csm}}, [&](void* const* d) {
        return ds_csm_spec_dev(c, (const ds_c32*)d[0], n_bins, n_frames, n_ch, amp_sqrt, norm_scale, factor, halve_edges,
                               (ds_c32*)d[1]);
    });
}

// ---- delay-and-sum beamformer map ---------------------------------------------------
static int das_map_check(ds_ctx* c, const void* csm, const void* h, const void* map, int n_bins, int n_ch, int n_grid) {
    if (!c || !csm || !h || !map) return fail(c, DS_ERR_ARG, "ds_das_map: null argument");
    if (n_bins <= 0 || n_ch <= 0 || n_grid <= 0) return fail(c, DS_ERR_ARG, "ds_das_map: bad shape");
    return DS_OK;
}

extern "C" int ds_das_map_dev(ds_ctx* c, const ds_c32* csm, const ds_c32* h, int n_bins, int n_ch,
                              int n_grid, float* map) {
    CHK(das_map_check(c, csm, h, map, n_bins, n_ch, n_grid));
    if (n_bins > 65535) return fail(c, DS_ERR_UNSUP, "ds_das_map: more than 65535 bins per call is not built yet");
    DasArgs a{(const float2*)csm, (const float2*)h, n_bins, n_ch, n_grid, map};
    CHK(launch(c, "das_map", k_das_map, dim3((n_grid + 127) / 128, n_bins), 256, 0, a));
    return DS_OK;
}

__global__ void k_csm_das_prepare(const float2* in, int64_t total, int n_ch, float scale, int zero_diag, float2* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t e = i % ((int64_t)n_ch * n_ch);
    const bool diag = zero_diag && (e / n_ch == e % n_ch);
    const float2 v = in[i];
    out[i] = diag ? make_float2(0.f, 0.f) : make_float2(v.x * scale, v.y * scale);
}
extern "C" int ds_csm_das_prepare_dev(ds_ctx* c, const ds_c32* csm, int n_bins, int n_ch, double scale,
                                      int zero_diagonal, ds_c32* out) {
    if (!c || !csm || !out) return fail(c, DS_ERR_ARG, "ds_csm_das_prepare: null argument");
    if (n_bins <= 0 || n_ch <= 0) return fail(c, DS_ERR_ARG, "ds_csm_das_prepare: bad shape");
    const int64_t total = (int64_t)n_bins * n_ch * n_ch;
    hipLaunchKernelGGL(k_csm_das_prepare, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, (const float2*)csm,
                       total, n_ch, (float)scale, zero_diagonal, (float2*)out);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}
extern "C" int ds_das_map(ds_ctx* c, const ds_c32* csm, const ds_c32* h, int n_bins, int n_ch, int n_grid,
                          float* map) {
    CHK(das_map_check(c, csm, h, map, n_bins, n_ch, n_grid));
    const size_t nc = (size_t)n_bins * n_ch * n_ch, nh = (size_t)n_bins * n_ch * n_grid, nm = (size_t)n_grid * n_bins;
    return staged(c, {{8, nc, csm, nullptr}, {8, nh, h, nullptr}, {4, nm, nullptr, map}}, [&](void* const* d) {
        return ds_das_map_dev(c, (const ds_c32*)d[0], (const ds_c32*)d[1], n_bins, n_ch, n_grid, (float*)d[2]);
    });
}

// ---- MVDR / Functional / Orthogonal / CLEAN-SC beamformer maps (kernels_beamform.hpp) -----------
// what every entry of this family and its _dev twin refuse: a null context or array (in, in2, out: the host's or the
// device's), a bad shape, a matrix or a grid beyond the kernels
static int bf_check(ds_ctx* c, const char* who, const void* in, const void* in2, const void* out, int n_bins, int n_ch,
                    int n_grid) {
    if (!c || !in || !in2 || !out) return fail(c, DS_ERR_ARG, who, "null argument");
    if (n_bins <= 0 || n_ch <= 0 || n_grid <= 0) return fail(c, DS_ERR_ARG, who, "bad shape");
    if (n_ch > bf::MAX_CH)
        return fail(c, DS_ERR_UNSUP, who, "more than 64 microphones is not built (one bin's C x C "
                                          "complex128 matrix is held in LDS; C <= 64)");
    if (n_bins > 65535) return fail(c, DS_ERR_UNSUP, who, "more than 65535 bins per call is not built yet");
    return DS_OK;
}

extern "C" int ds_bf_eigh_dev(ds_ctx* c, const double* a, int n_bins, int n_ch, double* w, double* v) {
    CHK(bf_check(c, "ds_bf_eigh", a, w, v, n_bins, n_ch, 1));
    bf::EighArgs ea{(const double2*)a, n_ch, w, (double2*)v};
    return launch(c, "bf_eigh", bf::k_bf_eigh, dim3(n_bins), bf::THREADS, 0, ea);
}

extern "C" int ds_bf_eigh(ds_ctx* c, const double* a, int n_bins, int n_ch, double* w, double* v) {
    CHK(bf_check(c, "ds_bf_eigh", a, w, v, n_bins, n_ch, 1));
    const size_t nm = (size_t)n_bins * n_ch * n_ch, nw = (size_t)n_bins * n_ch;
    return staged(c, {{16, nm, a, nullptr}, {16, nm, nullptr, v}, {8, nw, nullptr, w}}, [&](void* const* d) {
        return ds_bf_eigh_dev(c, (const double*)d[0], n_bins, n_ch, (double*)d[2], (double*)d[1]);
    });
}

extern "C" int ds_bf_eig_map_dev(ds_ctx* c, const double* csm, const double* h, int n_bins, int n_ch, int n_grid,
                                 int method, double gamma, int n_eig, double* map) {
    CHK(bf_check(c, "ds_bf_eig_map", csm, h, map, n_bins, n_ch, n_grid));
    if (method != bf::MVDR && method != bf::FUNCTIONAL && method != bf::ORTHOGONAL)
        return fail(c, DS_ERR_ARG, "ds_bf_eig_map: method must be 0 (MVDR), 1 (Functional) or 2 (Orthogonal)");
    if (method == bf::ORTHOGONAL && (n_eig <= 0 || n_eig > n_ch))
        return fail(c, DS_ERR_ARG, "ds_bf_eig_map: n_eig must be in [1, n_ch]");
    if (method != bf::ORTHOGONAL) n_eig = 0;
    const size_t nm = (size_t)n_bins * n_ch * n_ch, nw = (size_t)n_bins * n_ch, np = (size_t)n_bins * n_eig * n_grid;
    double2* dv;
    double *dw, *dp;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        dv = cv.take<double2>(nm);
        dw = cv.take<double>(nw);
        dp = np ? cv.take<double>(np) : nullptr;
    }));
    CHK(ds_bf_eigh_dev(c, csm, n_bins, n_ch, dw, (double*)dv));
    bf::ProjArgs pa{dw, dv, (const double2*)h, n_ch, n_grid, n_bins, method, n_eig, gamma, map, dp};
    CHK(launch(c, "bf_project", bf::k_bf_project, dim3((n_grid + bf::THREADS - 1) / bf::THREADS, n_bins),
               bf::THREADS, 0, pa));
    if (method == bf::ORTHOGONAL) CHK(launch(c, "bf_orth_pick", bf::k_bf_orth_pick, dim3(n_bins), bf::THREADS, 0, pa));
    return DS_OK;
}

extern "C" int ds_bf_eig_map(ds_ctx* c, const double* csm, const double* h, int n_bins, int n_ch, int n_grid,
                             int method, double gamma, int n_eig, double* map) {
    CHK(bf_check(c, "ds_bf_eig_map", csm, h, map, n_bins, n_ch, n_grid));
    const size_t nc = (size_t)n_bins * n_ch * n_ch, nh = (size_t)n_bins * n_ch * n_grid, nm = (size_t)n_grid * n_bins;
    return staged(c, {{16, nc, csm, nullptr}, {16, nh, h, nullptr}, {8, nm, nullptr, map}}, [&](void* const* d) {
        return ds_bf_eig_map_dev(c, (const double*)d[0], (const double*)d[1], n_bins, n_ch, n_grid, method, gamma, n_eig,
                                 (double*)d[2]);
    });
}

extern "C" int ds_bf_cleansc_dev(ds_ctx* c, const double* csm, const double* h, int n_bins, int n_ch, int n_grid,
                                 int max_iter, double safety, int remove_diagonal, double* map) {
    CHK(bf_check(c, "ds_bf_cleansc", csm, h, map, n_bins, n_ch, n_grid));
    if (max_iter <= 0) return fail(c, DS_ERR_ARG, "ds_bf_cleansc: max_iter must be positive");
    if (!(safety > 0.0 && safety <= 1.0)) return fail(c, DS_ERR_ARG, "ds_bf_cleansc: safety factor must be in (0, 1]");
    double* dr;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) { dr = cv.take<double>((size_t)n_bins * n_grid); }));
    bf::CleanArgs ca{(const double2*)csm, (const double2*)h, n_ch, n_grid, n_bins, max_iter, remove_diagonal ? 1 : 0,
                     safety, dr, map};
    return launch(c, "bf_cleansc", bf::k_bf_cleansc, dim3(n_bins), bf::THREADS, 0, ca);
}

extern "C" int ds_bf_cleansc(ds_ctx* c, const double* csm, const double* h, int n_bins, int n_ch, int n_grid,
                             int max_iter, double safety, int remove_diagonal, double* map) {
    CHK(bf_check(c, "ds_bf_cleansc", csm, h, map, n_bins, n_ch, n_grid));
    const size_t nc = (size_t)n_bins * n_ch * n_ch, nh = (size_t)n_bins * n_ch * n_grid, nm = (size_t)n_grid * n_bins;
    return staged(c, {{16, nc, csm, nullptr}, {16, nh, h, nullptr}, {8, nm, nullptr, map}}, [&](void* const* d) {
        return ds_bf_cleansc_dev(c, (const double*)d[0], (const double*)d[1], n_bins, n_ch, n_grid, max_iter, safety,
                                 remove_diagonal, (double*)d[2]);
    });
}

// ---- FIR ---------------------------------------------------------------------
// One call of ds_fir_ola_dev, checked by fir_check (`who`: the entry called); the runners apply the parallel mode
struct FirCall {
    const char* who;
    const float* x; int n_ch; int64_t ldx, n_samples; const float* taps; int n_filt, n_taps, mode; float* y; int64_t ld_y;
};
static int fir_check(ds_ctx* c, const FirCall& f) {
    if (!c || !f.x || !f.taps || !f.y) return fail(c, DS_ERR_ARG, f.who, "null argument");
    if (f.n_ch <= 0 || f.n_samples <= 0 || f.n_filt <= 0 || f.n_taps <= 0 || f.ldx < f.n_samples || f.ld_y < f.n_samples)
        return fail(c, DS_ERR_ARG, f.who, "bad shape");
    if (!fb_mode_ok(f.mode)) return fail(c, DS_ERR_ARG, f.who, "invalid filter bank apply mode");
    return DS_OK;
}

static int fir_block_len(int n_taps, int v = 0) {  // v: forced block length (DSPTOOLBOX_AMD_FIR_BLOCK), 0 = none
    int n = 1024;
    while (n < 4 * n_taps && n < kMaxFft) n <<= 1;
    // 1025 .. 2048 taps would take generic 8192-point blocks (75 % of every block new samples): the
    // register kernel for 16384-point blocks with its whole-group stores is faster (1025 taps:
    // 2.06 -> 1.57 ms on the 32-band x 8 x 2^22 shape) when the discarded length is a multiple of 4
    if (n == 8192 && ((n_taps - 1) & 3) == 0) n = 16384;
    if (v >= 1024 && v <= kMaxFft && is_pow2(v) && n_taps - 1 <= v / 2) n = v;  // DSPTOOLBOX_AMD_FIR_BLOCK
    return n;
}

// a signal shorter than the filter (or a tiny one): the direct sum in float64 -- no rounding floor set by the block's
// peak, which is what an FFT convolution leaves on an output far below (peak of the block) x (size of the taps)
// (kernels_freqz.hpp; DESIGN section 2, limit (x))
static int fir_direct_run(ds_ctx* c, const FirCall& f) {
    freqz::DirectArgs a{f.x, f.taps, f.n_samples, f.ldx, f.ld_y, f.n_ch, f.n_taps, f.y};
    return launch(c, "fir@direct_f64", freqz::k_fir_direct, dim3((unsigned)((f.n_samples + 255) / 256), f.n_ch, f.n_filt), 256,
                  0, a);
}

// Up to 4097 taps: uniformly partitioned overlap-save on the 4096-point register transform, three independent
// workgroups per CU (kernels_fir4k.hpp; two partitions: k_fir3 since round 5, DSPTOOLBOX_AMD_FIR_3PERCU=0 keeps the
// two-per-CU k_fir<2> with its tap-spectrum prefetch).
static int fir4k_run(ds_ctx* c, const FirCall& f) {
    namespace f4 = fir4k;
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    const int P = f4::partitions(f.n_taps);
    float4* hp;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) { hp = cv.take<float4>((size_t)f.n_filt * P * 8 * 256); }));
    f4::TapArgs ta{f.taps, f.n_filt, f.n_taps, P, c->w4_tables, hp};
    CHK(launch(c, "fir_taps", f4::k_taps, dim3((unsigned)(f.n_filt * P)), f4::NT, f4::LDS_BYTES, ta));
    const int pairs = (f.n_ch + 1) / 2;
    const int n_blocks = (int)((f.n_samples + f4::HOP - 1) / f4::HOP);
    // every workgroup resident at once (3 or 2 per CU): a run of blocks each, one extra forward
    // transform per run with two partitions
    const bool three = P == 2 && c->cfg.fir_3percu && !c->cfg.fir_stage;
    int chunks = std::max(1, ((P == 1 || three) ? 768 : 512) / pairs);
    if (c->cfg.fir_chunks > 0) chunks = c->cfg.fir_chunks;
    chunks = std::min(chunks, n_blocks);
    f4::Args a{f.x, f.n_samples, f.ldx, f.ld_y, f.n_ch, f.n_filt, n_blocks, chunks, c->w4_tables, hp, f.y};
    const dim3 grid((unsigned)(pairs * chunks));
    if (c->cfg.fir_stage) {  // round-5 experiment: stores through a per-wave LDS strip (profiles/r05_fir_staged_stores.txt)
        if (P == 1) return launch(c, "fir@4k_p1_staged", f4::k_fir<1, true>, grid, f4::NT, f4::LDS_BYTES + f4::STAGE_BYTES, a);
        return launch(c, "fir@4k_p2_staged", f4::k_fir<2, true>, grid, f4::NT, f4::LDS_BYTES + f4::STAGE_BYTES, a);
    }
    if (P == 1) return launch(c, "fir@4k_p1", f4::k_fir<1>, grid, f4::NT, f4::LDS_BYTES, a);
    if (three) return launch(c, "fir@4k_p2_3percu", f4::k_fir3<0>, grid, f4::NT, f4::LDS_BYTES, a);
    return launch(c, "fir@4k_p2", f4::k_fir<2>, grid, f4::NT, f4::LDS_BYTES, a);
}

// tap spectra of N-point blocks, hs[n_filt][N] (perm: room for their permuted copy behind them)
static int fir_block_taps(ds_ctx* c, const FirCall& f, int N, bool perm, const float2** tw, float2** hs, float2** hperm) {
    CHK(get_twiddles(c, N, tw));
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        *hs = cv.take<float2>((size_t)f.n_filt * N);
        *hperm = perm ? cv.take<float2>((size_t)f.n_filt * N) : nullptr;
    }));
    FirTapsArgs a{f.taps, f.n_filt, f.n_taps, *tw, *hs};
    DISPATCH_N(N, CHK(launch(c, "fir_taps", k_fir_taps<NN>, dim3((f.n_filt + 1) / 2), Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, a)));
    return DS_OK;
}

// 16384-point blocks: four 4096-point register transforms per block (kernels_fir16k.hpp)
static int fir16k_run(ds_ctx* c, const FirCall& f) {
    const int N = fir16k::NBIG;
    const float2* tw;
    float2 *hs, *hperm;
    CHK(fir_block_taps(c, f, N, true, &tw, &hs, &hperm));
    const int L = N - (f.n_taps - 1);
    const int64_t n_blocks = (f.n_samples + L - 1) / L;
    const int pairs = (f.n_ch + 1) / 2;
    CHK(ensure_table(c, &c->w4_tables, welch4096::host_tables));
    CHK(ensure_table(c, &c->fir16k_tables, fir16k::host_tables));
    fir16k::PermArgs pa{hs, f.n_filt, hperm};
    CHK(launch(c, "fir_taps", fir16k::k_permute, dim3((unsigned)(((int64_t)f.n_filt * N + 255) / 256)), 256, 0, pa));
    fir16k::Args a{f.x, f.n_samples, f.ldx, f.ld_y, f.n_ch, f.n_filt, f.n_taps, c->w4_tables, c->fir16k_tables, hperm, f.y, 0};
    // interior blocks of a 4097-tap filter with 16-byte aligned rows: the store-everything variant
    int64_t n_plain = 0;
    if (((f.n_taps - 1) & 3) == 0 && (f.ld_y & 3) == 0 && (((uintptr_t)f.y) & 15) == 0) n_plain = f.n_samples / L;
    const bool ragged = n_blocks > n_plain;
    if (n_plain == 0) {
        return launch(c, "fir@16k_ragged", fir16k::k_fir<false>, dim3((unsigned)n_blocks, pairs), fir16k::NTB,
                      fir16k::LDS_BYTES, a);
    }
    // The few ragged blocks go to the side stream so they run beside the main grid's last,
    // partly filled round instead of after it (fork after the tap spectra, join at the end).
    if (ragged) {
        HIPCHK(c, hipFuncSetAttribute((const void*)fir16k::k_fir<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)fir16k::LDS_BYTES));
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
        fir16k::Args ar = a;
        ar.block0 = (int)n_plain;
        hipLaunchKernelGGL(fir16k::k_fir<false>, dim3((unsigned)(n_blocks - n_plain), pairs), dim3(fir16k::NTB),
                           fir16k::LDS_BYTES, c->side, ar);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev_join, c->side));
    }
    // one workgroup per CU: split the filter loop over 1, 2 or 4 workgroups per block when that
    // fills the last round better (cost ~ rounds x (filters per slice + 1 forward transform))
    int split = 1;
    for (int64_t s = 1, best = -1, wgs = n_plain * pairs; s <= 4 && s <= f.n_filt; s *= 2) {
        const int64_t cost = ((wgs * s + 255) / 256) * ((f.n_filt + s - 1) / s + 1);
        if (best < 0 || cost < best) best = cost, split = (int)s;
    }
    if (c->cfg.fir_split > 0) split = std::min(c->cfg.fir_split, f.n_filt);
    CHK(launch(c, "fir@16k", fir16k::k_fir<true>, dim3((unsigned)n_plain, pairs, split), fir16k::NTB, fir16k::LDS_BYTES, a));
    if (ragged) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return DS_OK;
}

// Long filters (more taps than half the largest LDS-resident block): overlap-save on the
// four-step FFT with blocks of 2^15 .. 2^24 points.  Per block: one forward transform of the
// channel pairs, then groups of filters: multiply by the tap spectra, inverse, store.
static int fir_long_run(ds_ctx* c, const FirCall& f) {
    const int n_ch = f.n_ch, n_filt = f.n_filt, n_taps = f.n_taps;
    const int64_t n_samples = f.n_samples;
    if ((int64_t)n_taps - 1 > kMaxBigFft / 2)
        return fail(c, DS_ERR_UNSUP, std::string(f.who) + ": more than 2^23 + 1 taps is not built yet");
    int64_t L = (int64_t)1 << 15;
    while (L < 4 * (int64_t)n_taps && L < kMaxBigFft) L <<= 1;
    while (L > ((int64_t)1 << 15) && L / 2 >= n_samples + n_taps - 1) L >>= 1;  // short signals: one block
    const int64_t nb = L / 2 + 1, step = L - (n_taps - 1);
    const int npair = (n_ch + 1) / 2;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(n_filt, ((int64_t)1 << 25) / (npair * L)));
    const size_t scratch = (size_t)G * npair * L;
    float2 *R, *Qs, *P, *S;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        R = cv.take<float2>((size_t)n_filt * nb);
        Qs = cv.take<float2>((size_t)npair * L);
        P = cv.take<float2>(scratch);
        S = cv.take<float2>(scratch);
    }));
    // tap spectra R[k][nb], 2*G*npair filters per pass through the scratch buffers
    for (int k0 = 0; k0 < n_filt; k0 += 2 * G * npair) {
        const int nf = std::min(2 * G * npair, n_filt - k0), bt = (nf + 1) / 2;
        CHK(big_cols(c, nullptr, f.taps + (int64_t)k0 * n_taps, nf, n_taps, n_taps, P, L, bt));
        CHK(big_rows(c, P, S, L, bt));
        dsbig::UnpackArgs u{S, L, nf, 1.0f, R + (int64_t)k0 * nb, 1, nb};
        CHK(launch(c, "bigfft_unpack", dsbig::k_big_unpack, dim3(1024, bt), 256, 0, u));
    }
    for (int64_t b0 = 0; b0 < n_samples; b0 += step) {
        CHK(launch_big_cols(c, {nullptr, f.x, nullptr, n_samples, 0, P, L, 0, 0, 0, f.ldx, n_ch, nullptr,
                                nullptr, nullptr, 0, 0, 0, 0, 0, b0 - (n_taps - 1)}, npair));
        CHK(big_rows(c, P, Qs, L, npair));  // spectrum of the block, kept while the filter groups reuse P / S
        const int64_t n_out = std::min<int64_t>(step, n_samples - b0);
        for (int k0 = 0; k0 < n_filt; k0 += G) {
            const int g = std::min(G, n_filt - k0), bt = g * npair;
            dsbig::MulBankArgs m{Qs, R + (int64_t)k0 * nb, P, L, npair};
            CHK(launch(c, "bigfft_mul", dsbig::k_big_mul_bank, dim3(1024, bt), 256, 0, m));
            CHK(big_cols(c, P, nullptr, n_ch, 0, 0, P, L, bt));
            CHK(big_rows(c, P, S, L, bt));
            dsbig::StoreArgs st{S, L, n_out, f.ld_y, n_ch, f.y + (int64_t)k0 * n_ch * f.ld_y + b0, (int64_t)n_taps - 1};
            CHK(launch(c, "bigfft_store", dsbig::k_big_store, dim3(1024, bt), 256, 0, st));
        }
    }
    return DS_OK;
}

// every other block length: the LDS-resident transform (kernels_generic.hpp)
static int fir_generic_run(ds_ctx* c, const FirCall& f) {
    const int N = fir_block_len(f.n_taps, c->cfg.fir_block);
    const float2* tw;
    float2 *hs, *hperm;
    CHK(fir_block_taps(c, f, N, false, &tw, &hs, &hperm));
    const int L = N - (f.n_taps - 1);
    FirArgs a{f.x, f.n_samples, f.ldx, f.ld_y, f.n_ch, f.n_filt, f.n_taps, tw, hs, f.y};
    const dim3 grid((unsigned)((f.n_samples + L - 1) / L), (f.n_ch + 1) / 2);
    DISPATCH_N(N, CHK(launch(c, "fir@generic", k_fir<NN>, grid, Cfg<NN>::NT, Cfg<NN>::LDS_BYTES, a)));
    return DS_OK;
}

using FirRunner = int (*)(ds_ctx*, const FirCall&);
// The kernel family of a checked parallel-mode call.
static FirRunner fir_route(const ds_ctx* c, const FirCall& f) {
    // The direct sum: at most 2^28 multiply-adds, every output sample one thread's sum over min(n_samples, n_taps)
    // products, at most 16384 of them (a 2^20-tap filter on 256 samples would be 256 threads of a million dependent steps
    // each).  DSPTOOLBOX_AMD_FIR_DIRECT=0 turns the route off (A/B against the FFT routes on the same shape).
    const int64_t terms = std::min<int64_t>(f.n_samples, f.n_taps);
    if (c->cfg.fir_direct && (f.n_samples < f.n_taps || f.n_samples <= 512) && terms <= 16384 &&
        f.n_samples * terms * f.n_ch * f.n_filt <= ((int64_t)1 << 28) && f.n_filt <= 65535 && f.n_ch <= 65535)
        return fir_direct_run;
    // DSPTOOLBOX_AMD_FIR_4K=0 keeps the block kernels below (A/B); =1 also sends the short filters to fir4k
    if (f.n_taps >= c->cfg.fir4k_min_taps && fir4k::partitions(f.n_taps) <= 2 && fir4k::fits(f.n_samples) && f.n_filt <= 16384)
        return fir4k_run;
    const int N = fir_block_len(f.n_taps, c->cfg.fir_block);
    if (f.n_taps - 1 > N / 2) return fir_long_run;
    return N == fir16k::NBIG && !c->cfg.fir_generic ? fir16k_run : fir_generic_run;
}

__global__ void k_sum_taps(const float* taps, int n_filt, int n_taps, float* out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_taps) return;
    double s = 0.0;
    for (int k = 0; k < n_filt; ++k) s += (double)taps[(int64_t)k * n_taps + t];
    out[t] = (float)s;
}

__global__ void k_taps_to_f64(const float* a, int n, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)a[i];
}
__global__ void k_f64_to_taps(const double* a, int n, float* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)a[i];
}
// out[n] = sum_k a[k] b[n-k], fp64 accumulate
__global__ void k_conv_taps(const double* a, int na, const float* b, int nb, double* out) {
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= na + nb - 1) return;
    int k0 = max(0, n - (nb - 1)), k1 = min(na - 1, n);
    double s = 0.0;
    for (int k = k0; k <= k1; ++k) s += a[k] * (double)b[n - k];
    out[n] = s;
}

// a checked call in any bank mode: the summed and sequential banks are parallel-mode calls with one filter
static int fir_bank(ds_ctx* c, const FirCall& f) {
    if (f.mode == DS_FB_PARALLEL) return fir_route(c, f)(c, f);
    const float* taps = f.taps;
    const int n_filt = f.n_filt, n_taps = f.n_taps;
    FirCall one = f;
    one.n_filt = 1;
    // (combined taps and the cascade's intermediate signal live in the context's aux scratch: no
    // allocation, free or synchronisation per call; everything stays ordered on the stream)
    if (f.mode == DS_FB_SUMMED) {
        // sum_k (x * b_k) = x * (sum_k b_k): one filter with the summed taps
        CHK(reserve(c, &c->aux, &c->aux_bytes, sizeof(float) * (size_t)n_taps));
        float* bs = (float*)c->aux;
        hipLaunchKernelGGL(k_sum_taps, dim3((n_taps + 255) / 256), dim3(256), 0, c->stream, taps, n_filt, n_taps, bs);
        HIPCHK(c, hipGetLastError());
        one.taps = bs;
        return fir_route(c, one)(c, one);
    }
    // ((x*b1)[:N]*b2)[:N]... = (x*(b1*b2*...))[:N] for causal filters: when the combined
    // response fits one block transform, convolve the taps (fp64, on the device) and
    // filter once -- no fp32 round trip of the intermediate signals through HBM.
    const int64_t n_comb = (int64_t)n_filt * (n_taps - 1) + 1;
    if (n_filt > 1 && n_comb - 1 <= kMaxBigFft / 2 && (double)n_comb * n_taps <= 1.0e10) {
        double *pa, *pb;
        float* bf;
        CHK(carve(c, &c->aux, &c->aux_bytes, [&](Carver& cv) {
            pa = cv.take<double>((size_t)n_comb);
            pb = cv.take<double>((size_t)n_comb);
            bf = cv.take<float>((size_t)n_comb);
        }));
        hipLaunchKernelGGL(k_taps_to_f64, dim3((n_taps + 255) / 256), dim3(256), 0, c->stream, taps, n_taps, pa);
        int len = n_taps;
        for (int k = 1; k < n_filt; ++k) {
            int nl = len + n_taps - 1;
            hipLaunchKernelGGL(k_conv_taps, dim3((nl + 255) / 256), dim3(256), 0, c->stream, pa, len,
                               taps + (int64_t)k * n_taps, n_taps, pb);
            std::swap(pa, pb);
            len = nl;
        }
        hipLaunchKernelGGL(k_f64_to_taps, dim3((len + 255) / 256), dim3(256), 0, c->stream, pa, len, bf);
        HIPCHK(c, hipGetLastError());
        one.taps = bf;
        one.n_taps = len;
        return fir_route(c, one)(c, one);
    }
    // long cascades: stage by stage, each truncated to n_samples like the reference loop
    float* tmp = nullptr;
    if (n_filt > 1) {
        CHK(reserve(c, &c->aux, &c->aux_bytes, sizeof(float) * (size_t)f.n_ch * f.n_samples));
        tmp = (float*)c->aux;
    }
    for (int k = 0; k < n_filt; ++k) {
        float* dst = ((n_filt - 1 - k) % 2 == 0) ? f.y : tmp;  // ping-pong, last stage lands in y
        one.taps = taps + (int64_t)k * n_taps;
        one.y = dst;
        one.ld_y = (dst == f.y) ? f.ld_y : f.n_samples;
        CHK(fir_route(c, one)(c, one));
        one.x = dst;
        one.ldx = one.ld_y;
    }
    return DS_OK;
}

extern "C" int ds_fir_ola_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_samples,
                              const float* taps, int n_filt, int n_taps, int mode, float* y,
                              int64_t ld_y) {
    const FirCall f{"ds_fir_ola_dev", x, n_ch, ldx, n_samples, taps, n_filt, n_taps, mode, y, ld_y};
    CHK(fir_check(c, f));
    return fir_bank(c, f);
}

// ---- host-pointer entry points -------------------------------------------------
// Each stages its arrays in ctx->io around the _dev entry.  The *_f64 entries take the reference's own float64 layouts
// and cross the boundary through the pinned pipelines below; the others copy planar fp32 arrays as they are.

// Fused boundary upload: (samples, channels) float64 C-order host array -> planar float32 device
// rows.  Chunks of samples are cast + transposed by host threads straight into one of two pinned
// buffers and sent with an asynchronous 2-D copy, so the cast of chunk k+1 overlaps the DMA of
// chunk k (a pageable hipMemcpy of the pre-cast array moves ~13 GB/s; this path is bound by the
// threads' cast, ~35 GB/s of float64 input).
static const size_t kPinBytes = (size_t)32 << 20;
// The transport of the pipelines in host_marshal.hpp: asynchronous copies on the context's stream, one
// event per pinned staging chunk.
struct HipTransport {
    ds_ctx* c;
    hipError_t err = hipSuccess;
    bool ok(hipError_t e) {
        if (e != hipSuccess) err = e;
        return e == hipSuccess;
    }
    bool mark(int b) {
        if (!ok(hipEventRecord(c->pin_ev[b], c->stream))) return false;
        c->pin_busy[b] = true;
        return true;
    }
    bool wait(int b) {
        if (c->pin_busy[b] && !ok(hipEventSynchronize(c->pin_ev[b]))) return false;
        c->pin_busy[b] = false;
        return true;
    }
    bool h2d_2d(float* dst, size_t dpitch, const float* src, size_t spitch, size_t width, size_t rows, int b) {
        return ok(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyHostToDevice, c->stream)) && mark(b);
    }
    bool d2h_2d(float* dst, size_t dpitch, const float* src, size_t spitch, size_t width, size_t rows, int b) {
        return ok(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToHost, c->stream)) && mark(b);
    }
    bool d2h(float* dst, const float* src, size_t bytes, int b) {
        return ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)) && mark(b);
    }
    bool h2d(float* dst, const float* src, size_t bytes, int b) {
        return ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream)) && mark(b);
    }
};
// One run of a host_marshal.hpp pipeline, pipe(transport, pinned chunks), on the context's two pinned chunks
// (allocated on first use; drain: wait for their pending copies first).  `what` names the pipeline in errors.
template <class F>
static int pinned(ds_ctx* c, bool drain, const char* what, F&& pipe) {
    for (int i = 0; i < 2; ++i) {
        if (!c->pin[i]) {
            HIPCHK(c, hipHostMalloc(&c->pin[i], kPinBytes, hipHostMallocDefault));
            HIPCHK(c, hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming));
        }
        if (drain && c->pin_busy[i]) {
            HIPCHK(c, hipEventSynchronize(c->pin_ev[i]));
            c->pin_busy[i] = false;
        }
    }
    HipTransport tr{c};
    float* const pin[2] = {(float*)c->pin[0], (float*)c->pin[1]};
    if (pipe(tr, pin)) return DS_OK;
    if (tr.err != hipSuccess) return fail(c, DS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(tr.err));
    return fail(c, DS_ERR_UNSUP, std::string(what) + ": too many channels for the staging chunk");
}
static int upload_narrow_f64(ds_ctx* c, const double* src, int64_t n, float* dst_dev) {
    return pinned(c, false, "upload_narrow_f64", [&](HipTransport& tr, float* const* pin) {
        return dshost::upload_narrow(tr, pin, kPinBytes, src, n, dst_dev);
    });
}
static int download_widen(ds_ctx* c, const float* src_dev, int64_t n, double* dst) {
    return pinned(c, true, "download_widen", [&](HipTransport& tr, float* const* pin) {
        return dshost::download_widen(tr, pin, kPinBytes, src_dev, n, dst);
    });
}
static int download_interleave(ds_ctx* c, const float* src_dev, int64_t n_samples, int n_ch, int64_t ld,
                               double* dst) {
    return pinned(c, true, "download_interleave", [&](HipTransport& tr, float* const* pin) {
        return dshost::download_interleave(tr, pin, kPinBytes, src_dev, n_samples, n_ch, ld, dst);
    });
}
// a signal into planar float32 rows dst[n_ch][n_samples]: x has that layout already; x64 is the reference's
// (n_samples, n_ch) float64 C-order array
static int upload_signal(ds_ctx* c, const float* x, const double* x64, int64_t n_samples, int n_ch, float* dst) {
    if (!x64) return ds_upload(c, dst, x, sizeof(float) * (size_t)n_ch * n_samples);
    return pinned(c, false, "upload_planar_f64", [&](HipTransport& tr, float* const* pin) {
        return dshost::upload_planar(tr, pin, kPinBytes, x64, n_samples, n_ch, dst, n_samples);
    });
}

// The bodies below serve both entries of a pair: x / x64 as upload_signal, outputs as ds_c32 / float or, with the
// *64 pointer, as the reference's complex128 / float64 layouts.  `who` is the entry's name in its error messages.

// out: the (bins, frames, channels) spectrogram
static int stft_host(ds_ctx* c, const char* who, const float* x, const double* x64, int64_t n_samples, int n_ch, int W,
                     int hop, int nfft, int64_t pad_front, int n_frames, const float* window, int detrend, float scale,
                     float edge_scale, int power, ds_c32* out, double* out64) {
    // (the host pointers, only checked: the staged copies replace them below)
    StftCall s{who, x ? x : (const float*)x64, n_samples, n_ch, n_samples, W, hop, nfft, pad_front, n_frames, window,
               detrend, scale, edge_scale, power, out ? (float2*)out : (float2*)out64};
    CHK(stft_check(c, s));
    const size_t no = (size_t)(nfft / 2 + 1) * n_frames * n_ch;
    float *dx, *dw;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        s.x = dx = cv.take<float>((size_t)n_ch * n_samples);
        s.window = dw = cv.take<float>(W);
        s.out = cv.take<float2>(no);
    }));
    CHK(upload_signal(c, x, x64, n_samples, n_ch, dx));
    CHK(ds_upload(c, dw, window, (size_t)W * 4));
    CHK(stft_route(c, s)(c, s));
    if (out64) return download_widen(c, (const float*)s.out, (int64_t)no * 2, out64);
    return ds_download(c, out, s.out, no * 8);
}
extern "C" int ds_stft_r2c(ds_ctx* c, const float* x, int64_t n_samples, int n_ch, int W, int hop,
                           int nfft, int64_t pad_front, int n_frames, const float* window, int detrend,
                           float scale, float edge_scale, int power, ds_c32* out) {
    return stft_host(c, "ds_stft_r2c", x, nullptr, n_samples, n_ch, W, hop, nfft, pad_front, n_frames, window, detrend,
                     scale, edge_scale, power, out, nullptr);
}
// ds_stft_r2c with the reference's layouts on both sides: x (n_samples, n_ch) float64 C-order in,
// (bins, frames, channels) complex128 out.
extern "C" int ds_stft_r2c_f64(ds_ctx* c, const double* x, int64_t n_samples, int n_ch, int W, int hop,
                               int nfft, int64_t pad_front, int n_frames, const float* window, int detrend,
                               float scale, float edge_scale, int power, double* out_c128) {
    return stft_host(c, "ds_stft_r2c_f64", nullptr, x, n_samples, n_ch, W, hop, nfft, pad_front, n_frames, window,
                     detrend, scale, edge_scale, power, nullptr, out_c128);
}

// stft / stft64: the (bins, frames, channels) spectrogram as ds_c32 / complex128; out: (n_ch, total_length) float32
// rows, out64: the reference's (total_length, n_ch) float64 array
static int istft_host(ds_ctx* c, const char* who, const ds_c32* stft, const double* stft64, int n_bins, int n_frames,
                      int n_ch, int nfft, int W, int step, int frame_offset, int n_frames_total, const float* window,
                      float scale, int64_t total_length, float* out, double* out64) {
    // (the host pointers, only checked: the staged copies replace them below)
    IstftCall q{who, stft ? (const float2*)stft : (const float2*)stft64, n_bins, n_frames, n_ch, nfft, W, step,
                frame_offset, n_frames_total, window, scale, total_length, out ? out : (float*)out64, total_length};
    CHK(istft_check(c, q));
    const size_t ns = (size_t)n_bins * n_frames * n_ch, no = (size_t)n_ch * total_length;
    float2* ds;
    float* dw;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        q.stft = ds = cv.take<float2>(ns);
        q.window = dw = cv.take<float>(W);
        q.out = cv.take<float>(no);
    }));
    CHK(stft64 ? upload_narrow_f64(c, stft64, (int64_t)ns * 2, (float*)ds) : ds_upload(c, ds, stft, ns * 8));
    CHK(ds_upload(c, dw, window, (size_t)W * 4));
    CHK(istft_route(c, q)(c, q));
    if (out64) return download_interleave(c, q.out, total_length, n_ch, total_length, out64);
    return ds_download(c, out, q.out, no * 4);
}
extern "C" int ds_istft(ds_ctx* c, const ds_c32* stft, int n_bins, int n_frames, int n_ch, int nfft, int W,
                        int step, int frame_offset, int n_frames_total, const float* window, float scale,
                        int64_t total_length, float* out) {
    return istft_host(c, "ds_istft", stft, nullptr, n_bins, n_frames, n_ch, nfft, W, step, frame_offset, n_frames_total,
                      window, scale, total_length, out, nullptr);
}
// ds_istft with the reference's layouts on both sides: the spectrogram (bins, frames, channels) complex128 in,
// the signal (total_length, n_ch) float64 out (transforms.istft, transforms/transforms.py:444-586).
extern "C" int ds_istft_f64(ds_ctx* c, const double* stft_c128, int n_bins, int n_frames, int n_ch, int nfft, int W,
                            int step, int frame_offset, int n_frames_total, const float* window, float scale,
                            int64_t total_length, double* out) {
    return istft_host(c, "ds_istft_f64", nullptr, stft_c128, n_bins, n_frames, n_ch, nfft, W, step, frame_offset,
                      n_frames_total, window, scale, total_length, nullptr, out);
}

// spec: (bins, channels)
static int rfft_host(ds_ctx* c, const char* who, const float* x, const double* x64, int n_ch, int64_t n_samples,
                     int n_fft, float scale, ds_c32* spec, double* spec64) {
    // (the host pointers, only checked: the staged copies replace them below)
    XformCall q{who, x ? x : (const float*)x64, 1, n_ch, n_samples, n_samples, n_fft, scale,
                spec ? (float2*)spec : (float2*)spec64};
    CHK(xform_check(c, q, false));
    const size_t no = (size_t)(n_fft / 2 + 1) * n_ch;
    float* dx;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        q.x = dx = cv.take<float>((size_t)n_ch * n_samples);
        q.spec = cv.take<float2>(no);
    }));
    CHK(upload_signal(c, x, x64, n_samples, n_ch, dx));
    CHK(rfft_route(q)(c, q));
    if (spec64) return download_widen(c, (const float*)q.spec, (int64_t)no * 2, spec64);
    return ds_download(c, spec, q.spec, no * 8);
}
extern "C" int ds_rfft(ds_ctx* c, const float* x, int n_ch, int64_t n_samples, int n_fft, float scale,
                       ds_c32* spec) {
    return rfft_host(c, "ds_rfft", x, nullptr, n_ch, n_samples, n_fft, scale, spec, nullptr);
}
// ds_rfft with the reference's layouts on both sides: x (n_samples, n_ch) float64 C-order in, (bins, channels)
// complex128 out (Signal.get_spectrum with SpectrumMethod.FFT, classes/signal.py:899-911).
extern "C" int ds_rfft_f64(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, int n_fft, float scale,
                           double* spec_c128) {
    return rfft_host(c, "ds_rfft_f64", nullptr, x, n_ch, n_samples, n_fft, scale, nullptr, spec_c128);
}

// y: (n_items, n_ch, n_samples) float32, ir: (n_items, n_ch, n_out) float32; or one item in the reference's layouts,
// y64 (n_samples, n_ch) and ir64 (n_out, n_ch) float64
static int deconv_host(ds_ctx* c, const char* who, const float* y, const double* y64, int n_items, int n_ch,
                       int64_t n_samples, int n_fft, const ds_c32* r, int r_per_channel, int64_t n_out, float* ir,
                       double* ir64) {
    // (the host pointers, only checked: the staged copies replace them below)
    XformCall q{who, y ? y : (const float*)y64, n_items, n_ch, n_samples, n_samples, n_fft, 1.0f, nullptr,
                (const float2*)r, r_per_channel, n_out, n_out, ir ? ir : (float*)ir64};
    CHK(xform_check(c, q, true));
    const size_t nr = (size_t)(r_per_channel ? n_ch : 1) * (n_fft / 2 + 1), no = (size_t)n_items * n_ch * n_out;
    float* dy;
    float2* dr;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        q.x = dy = cv.take<float>((size_t)n_items * n_ch * n_samples);
        q.r = dr = cv.take<float2>(nr);
        q.ir = cv.take<float>(no);
    }));
    CHK(upload_signal(c, y, y64, n_samples, n_items * n_ch, dy));
    CHK(ds_upload(c, dr, r, nr * 8));
    CHK(deconv_route(c, q)(c, q));
    if (ir64) return download_interleave(c, q.ir, n_out, n_ch, n_out, ir64);
    return ds_download(c, ir, q.ir, no * 4);
}
extern "C" int ds_deconv(ds_ctx* c, const float* y, int n_items, int n_ch, int64_t n_samples, int n_fft,
                         const ds_c32* r, int r_per_channel, int64_t n_out, float* ir) {
    return deconv_host(c, "ds_deconv", y, nullptr, n_items, n_ch, n_samples, n_fft, r, r_per_channel, n_out, ir, nullptr);
}
// ds_deconv for ONE item in the reference's layouts: y (n_samples, n_ch) float64 in, the impulse responses
// (n_out, n_ch) float64 out (_spectral_deconvolve, transfer_functions/_transfer_functions.py:19-42).
extern "C" int ds_deconv_f64(ds_ctx* c, const double* y, int n_ch, int64_t n_samples, int n_fft, const ds_c32* r,
                             int r_per_channel, int64_t n_out, double* ir) {
    return deconv_host(c, "ds_deconv_f64", nullptr, y, 1, n_ch, n_samples, n_fft, r, r_per_channel, n_out, nullptr, ir);
}

// y: (bands or 1, n_ch, n_samples) float32, or y64: (bands or 1, n_samples, n_ch) float64
static int fir_ola_host(ds_ctx* c, const char* who, const float* x, const double* x64, int n_ch, int64_t n_samples,
                        const float* taps, int n_filt, int n_taps, int mode, float* y, double* y64) {
    // (the host pointers, only checked: the staged copies replace them below)
    FirCall f{who, x ? x : (const float*)x64, n_ch, n_samples, n_samples, taps, n_filt, n_taps, mode, y ? y : (float*)y64,
              n_samples};
    CHK(fir_check(c, f));
    const int n_out = mode == DS_FB_PARALLEL ? n_filt : 1;
    const size_t nt = (size_t)n_filt * n_taps, no = (size_t)n_out * n_ch * n_samples;
    float *dx, *dt;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        f.x = dx = cv.take<float>((size_t)n_ch * n_samples);
        f.taps = dt = cv.take<float>(nt);
        f.y = cv.take<float>(no);
    }));
    CHK(upload_signal(c, x, x64, n_samples, n_ch, dx));
    CHK(ds_upload(c, dt, taps, nt * 4));
    CHK(fir_bank(c, f));
    if (!y64) return ds_download(c, y, f.y, no * 4);
    for (int k = 0; k < n_out; ++k)
        CHK(download_interleave(c, f.y + (size_t)k * n_ch * n_samples, n_samples, n_ch, n_samples,
                                y64 + (size_t)k * n_samples * n_ch));
    return DS_OK;
}
extern "C" int ds_fir_ola(ds_ctx* c, const float* x, int n_ch, int64_t n_samples, const float* taps,
                          int n_filt, int n_taps, int mode, float* y) {
    return fir_ola_host(c, "ds_fir_ola", x, nullptr, n_ch, n_samples, taps, n_filt, n_taps, mode, y, nullptr);
}
// ds_fir_ola with the reference's layouts on both sides: x (n_samples, n_ch) float64 in,
// y (bands or 1, n_samples, n_ch) float64 out.
extern "C" int ds_fir_ola_f64(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, const float* taps,
                              int n_filt, int n_taps, int mode, double* y) {
    return fir_ola_host(c, "ds_fir_ola_f64", nullptr, x, n_ch, n_samples, taps, n_filt, n_taps, mode, nullptr, y);
}

// The body of the six host Welch entries: q with the host pointers (x / y planar float32 [n_ch][n_samples], or cast from
// x64 / y64: the reference's (n_samples, n_ch) float64 C-order arrays as they are, classes/signal.py:222-301)
static int welch_host(ds_ctx* c, WelchCall q, const double* x64, const double* y64) {
    // (the host pointers, only checked: the staged copies replace them below)
    CHK(welch_check(c, q));
    const float *hx = q.x, *hy = q.y, *hw = q.window;
    float2* const hc = q.out_c;
    float* const hr = q.out_r;
    const size_t no = (size_t)(q.W / 2 + 1) * q.n_out();
    float *dx, *dy, *dw;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        q.x = dx = cv.take<float>((size_t)q.n_cx * q.n_samples);
        if (hy) q.y = dy = cv.take<float>((size_t)q.n_cy * q.n_samples);
        q.window = dw = cv.take<float>(q.W);
        if (hc) q.out_c = cv.take<float2>(no);
        if (hr) q.out_r = cv.take<float>(no);
    }));
    CHK(upload_signal(c, hx, x64, q.n_samples, q.n_cx, dx));
    if (hy) CHK(upload_signal(c, hy, y64, q.n_samples, q.n_cy, dy));
    CHK(ds_upload(c, dw, hw, (size_t)q.W * 4));
    CHK(welch_route(c, q)(c, q));
    if (hc) CHK(ds_download(c, hc, q.out_c, no * 8));
    return hr ? ds_download(c, hr, q.out_r, no * 4) : DS_OK;
}
// ds_welch_tf with the reference's own array layout at the boundary: x (n_samples, n_cx) and
// y (n_samples, n_cy) float64 C-order (classes/signal.py:222-301), outputs as ds_welch_tf.
extern "C" int ds_welch_tf_f64(ds_ctx* c, const double* x, int n_cx, const double* y, int n_cy,
                               int64_t n_samples, int W, int hop, int n_frames, const float* window,
                               int detrend, int average, int mode, int amp_sqrt, double norm_scale,
                               double factor, int halve_edges, ds_c32* tf, float* coh) {
    return welch_host(c, {"ds_welch_tf_f64", TF, (const float*)x, n_cx, n_samples, (const float*)y, n_cy, n_samples, n_samples,
                          W, hop, n_frames, window, detrend, average, mode, amp_sqrt, norm_scale, factor, halve_edges,
                          (float2*)tf, coh}, x, y);
}
extern "C" int ds_welch_tf(ds_ctx* c, const float* x, int n_cx, const float* y, int n_cy,
                           int64_t n_samples, int W, int hop, int n_frames, const float* window,
                           int detrend, int average, int mode, int amp_sqrt, double norm_scale,
                           double factor, int halve_edges, ds_c32* tf, float* coh) {
    return welch_host(c, {"ds_welch_tf", TF, x, n_cx, n_samples, y, n_cy, n_samples, n_samples, W, hop, n_frames, window,
                          detrend, average, mode, amp_sqrt, norm_scale, factor, halve_edges, (float2*)tf, coh}, nullptr, nullptr);
}

extern "C" int ds_welch_psd(ds_ctx* c, const float* x, int n_cx, int64_t n_samples, int W, int hop,
                            int n_frames, const float* window, int detrend, int average, int amp_sqrt,
                            double norm_scale, double factor, int halve_edges, float* psd) {
    return welch_host(c, {"ds_welch_psd", PSD, x, n_cx, n_samples, nullptr, 0, 0, n_samples, W, hop, n_frames, window, detrend,
                          average, 0, amp_sqrt, norm_scale, factor, halve_edges, nullptr, psd}, nullptr, nullptr);
}
extern "C" int ds_welch_psd_f64(ds_ctx* c, const double* x, int n_cx, int64_t n_samples, int W, int hop,
                                int n_frames, const float* window, int detrend, int average, int amp_sqrt,
                                double norm_scale, double factor, int halve_edges, float* psd) {
    return welch_host(c, {"ds_welch_psd_f64", PSD, (const float*)x, n_cx, n_samples, nullptr, 0, 0, n_samples, W, hop, n_frames,
                          window, detrend, average, 0, amp_sqrt, norm_scale, factor, halve_edges, nullptr, psd}, x, nullptr);
}

// csd_i = mean_f conj(X_i) Y_i is the cross sum a transfer function with one input channel per
// output channel accumulates: the same kernels with the finish of kind CSD
extern "C" int ds_welch_csd(ds_ctx* c, const float* x, const float* y, int n_ch, int64_t n_samples,
                            int W, int hop, int n_frames, const float* window, int detrend,
                            int average, int amp_sqrt, double norm_scale, double factor,
                            int halve_edges, ds_c32* csd) {
    return welch_host(c, {"ds_welch_csd", CSD, x, n_ch, n_samples, y, n_ch, n_samples, n_samples, W, hop, n_frames, window,
                          detrend, average, 0, amp_sqrt, norm_scale, factor, halve_edges, (float2*)csd, nullptr}, nullptr, nullptr);
}
extern "C" int ds_welch_csd_f64(ds_ctx* c, const double* x, const double* y, int n_ch, int64_t n_samples,
                                int W, int hop, int n_frames, const float* window, int detrend,
                                int average, int amp_sqrt, double norm_scale, double factor,
                                int halve_edges, ds_c32* csd) {
    return welch_host(c, {"ds_welch_csd_f64", CSD, (const float*)x, n_ch, n_samples, (const float*)y, n_ch, n_samples, n_samples,
                          W, hop, n_frames, window, detrend, average, 0, amp_sqrt, norm_scale, factor, halve_edges,
                          (float2*)csd, nullptr}, x, y);
}

static int csm_host(ds_ctx* c, const char* who, const float* x, const double* x64, int n_ch, int64_t n_samples, int W,
                    int hop, int n_frames, const float* window, int detrend, int average, int amp_sqrt,
                    double norm_scale, double factor, int halve_edges, ds_c32* csm) {
    // (the host pointers, only checked: the staged copies replace them below)
    CsmCall q{who, x ? x : (const float*)x64, n_ch, n_samples, n_samples, W, hop, n_frames, window, detrend, average,
              amp_sqrt, norm_scale, factor, halve_edges, 0, W / 2 + 1, (float2*)csm};
    CHK(csm_check(c, q));
    const size_t no = (size_t)(W / 2 + 1) * n_ch * n_ch;
    float *dx, *dw;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        q.x = dx = cv.take<float>((size_t)n_ch * n_samples);
        q.window = dw = cv.take<float>(W);
        q.csm = cv.take<float2>(no);
    }));
    CHK(upload_signal(c, x, x64, n_samples, n_ch, dx));
    CHK(ds_upload(c, dw, window, (size_t)W * 4));
    CHK(csm_route(c, q)(c, q));
    return ds_download(c, csm, q.csm, no * 8);
}
extern "C" int ds_csm(ds_ctx* c, const float* x, int n_ch, int64_t n_samples, int W, int hop,
                      int n_frames, const float* window, int detrend, int average, int amp_sqrt,
                      double norm_scale, double factor, int halve_edges, ds_c32* csm) {
    return csm_host(c, "ds_csm", x, nullptr, n_ch, n_samples, W, hop, n_frames, window, detrend, average, amp_sqrt,
                    norm_scale, factor, halve_edges, csm);
}
extern "C" int ds_csm_f64(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, int W, int hop,
                          int n_frames, const float* window, int detrend, int average, int amp_sqrt,
                          double norm_scale, double factor, int halve_edges, ds_c32* csm) {
    return csm_host(c, "ds_csm_f64", nullptr, x, n_ch, n_samples, W, hop, n_frames, window, detrend, average, amp_sqrt,
                    norm_scale, factor, halve_edges, csm);
}

// ---- block-streaming FIR classes, state on the device (kernels_fir_stream.hpp) ----------
__global__ void k_stream_ones(float* dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = 1.f;
}
static int stream_ones(ds_ctx* c, float* dst, int n) {  // n_call unit impulses of length 1, written on the
                                                         // stream: a block step carries no host synchronisation
    hipLaunchKernelGGL(k_stream_ones, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, dst, n);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

extern "C" int ds_fir_part_step_dev(ds_ctx* c, float* inbuf, const float* block, int bs, int n_ch, int ch0,
                                    int n_call, const ds_c32* h, int n_part, int n_fir_ch, ds_c32* delay,
                                    int ind, float* out) {
    if (!c || !inbuf || !block || !h || !delay || !out) return fail(c, DS_ERR_ARG, "ds_fir_part_step: null argument");
    if (bs < 1 || n_ch < 1 || ch0 < 0 || n_call < 1 || ch0 + n_call > n_ch || n_part < 1 || ind < 0 || ind >= n_part ||
        (n_fir_ch != 1 && n_fir_ch != n_ch))
        return fail(c, DS_ERR_ARG, "ds_fir_part_step: bad shape");
    const int n_fft = 2 * bs, B = bs + 1;
    float2 *X, *Y;
    float *full, *ones;
    CHK(carve(c, &c->aux, &c->aux_bytes, [&](Carver& cv) {
        X = cv.take<float2>((size_t)B * n_call);
        Y = cv.take<float2>((size_t)B * n_call);
        full = cv.take<float>((size_t)n_call * n_fft);
        ones = cv.take<float>(n_call);
    }));
    CHK(stream_ones(c, ones, n_call));
    const int64_t nb = (int64_t)n_call * bs;
    hipLaunchKernelGGL(firstream::k_shift_in, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, c->stream, inbuf, block,
                       bs, ch0, n_call);
    HIPCHK(c, hipGetLastError());
    CHK(ds_rfft_dev(c, inbuf + (int64_t)ch0 * n_fft, n_call, n_fft, n_fft, n_fft, 1.0f, (ds_c32*)X));
    firstream::AccArgs aa{X, (float2*)delay, (const float2*)h, Y, B, n_part, n_ch, n_fir_ch, ch0, n_call, ind};
    const int64_t na = (int64_t)B * n_call;
    CHK(launch(c, "fir_part_acc", firstream::k_part_acc, dim3((unsigned)((na + 255) / 256)), 256, 0, aa));
    // numpy's irfft of bs + 1 bins without a length: 2 bs points
    CHK(ds_deconv_dev(c, ones, 1, n_call, 1, 1, n_fft, (const ds_c32*)Y, 1, n_fft, n_fft, full));
    hipLaunchKernelGGL(firstream::k_tail, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, c->stream,
                       (const float*)full, (int64_t)n_fft, bs, n_call, out);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

extern "C" int ds_fir_ols_step_dev(ds_ctx* c, float* row, const float* block, int bs, int64_t L,
                                   const ds_c32* h, float* out) {
    if (!c || !row || !block || !h || !out) return fail(c, DS_ERR_ARG, "ds_fir_ols_step: null argument");
    if (bs < 1 || L < 2 || bs > L || L > ((int64_t)1 << 22)) return fail(c, DS_ERR_ARG, "ds_fir_ols_step: bad shape");
    const int B = (int)(L / 2 + 1);
    const int64_t n_inv = 2 * (int64_t)(B - 1);  // L for even L, L - 1 for odd L: irfft without a length
    if (bs > n_inv) return fail(c, DS_ERR_ARG, "ds_fir_ols_step: block longer than the inverse transform");
    float2 *X, *Y;
    float *full, *roll, *one;
    CHK(carve(c, &c->aux, &c->aux_bytes, [&](Carver& cv) {
        X = cv.take<float2>(B);
        Y = cv.take<float2>(B);
        full = cv.take<float>((size_t)L);
        roll = cv.take<float>((size_t)L);
        one = cv.take<float>(1);
    }));
    CHK(stream_ones(c, one, 1));
    hipLaunchKernelGGL(firstream::k_ols_put, dim3((bs + 255) / 256), dim3(256), 0, c->stream, row, block, L, bs);
    HIPCHK(c, hipGetLastError());
    CHK(ds_rfft_dev(c, row, 1, L, L, (int)L, 1.0f, (ds_c32*)X));
    hipLaunchKernelGGL(firstream::k_cmul, dim3((B + 255) / 256), dim3(256), 0, c->stream, (const float2*)X,
                       (const float2*)h, Y, B);
    HIPCHK(c, hipGetLastError());
    CHK(ds_deconv_dev(c, one, 1, 1, 1, 1, (int)n_inv, (const ds_c32*)Y, 0, n_inv, n_inv, full));
    hipLaunchKernelGGL(firstream::k_tail, dim3((bs + 255) / 256), dim3(256), 0, c->stream, (const float*)full, n_inv, bs,
                       1, out);
    hipLaunchKernelGGL(firstream::k_ols_roll, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, c->stream,
                       (const float*)row, roll, L, bs);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(row, roll, sizeof(float) * (size_t)L, hipMemcpyDeviceToDevice, c->stream));
    return DS_OK;
}

// FIR transfer functions at arbitrary frequencies (host pointers; complex128 taps and result)
extern "C" int ds_fir_freqz(ds_ctx* c, const double* taps, int n_filt, int n_taps, const double* freqs_hz, int n_freq,
                            double fs_hz, double* out) {
    if (!c || !taps || !freqs_hz || !out) return fail(c, DS_ERR_ARG, "ds_fir_freqz: null argument");
    if (n_filt <= 0 || n_taps <= 0 || n_freq <= 0 || !(fs_hz > 0.0)) return fail(c, DS_ERR_ARG, "ds_fir_freqz: bad shape");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nt = (size_t)n_filt * n_taps, no = (size_t)n_filt * n_freq;
    return staged(c, {{16, nt, taps}, {8, (size_t)n_freq, freqs_hz}, {16, no, nullptr, out}}, [&](void* const* d) {
        freqz::Args a{(const double2*)d[0], n_filt, n_taps, (const double*)d[1], n_freq, fs_hz, (double2*)d[2]};
        return launch(c, "fir_freqz", freqz::k_freqz, dim3((n_freq + 255) / 256, n_filt), 256, 0, a);
    });
}

// ---- IIR filtering: cascades of second-order sections (kernels_iir.hpp) --------------------------------
// Host side of the carry: the normalised sections, the zero-input state transition A of each cascade and its
// powers Phi = A^L and Phi^B, in float64 (carry_tables.hpp).

// what the grids of the three passes hold, for every family on block_carry.hpp: a stream per block of grid y or x, a
// group of carry::G samples per block of grid x
static int carry_limits(ds_ctx* c, const char* who, int64_t n_streams, int64_t n_samples, const char* too_many_streams) {
    if (n_streams > 65535) return fail(c, DS_ERR_UNSUP, who, too_many_streams);
    if ((n_samples + carry::G - 1) / carry::G > INT32_MAX) return fail(c, DS_ERR_UNSUP, who, "signal too long");
    return DS_OK;
}

// sos [n_filt][n_sec][6] -> coef [n_filt][n_sec][5] (b0 b1 b2 a1 a2 / a0), phi = A^L, phig = A^(L B), each [n_filt][D][D]
static bool iir_tables(const double* sos, int n_filt, int n_sec, std::vector<double>& coef, std::vector<double>& phi,
                       std::vector<double>& phig) {
    const int d = 2 * n_sec;
    coef.assign((size_t)n_filt * n_sec * 5, 0.0);
    phi.assign((size_t)n_filt * d * d, 0.0);
    phig.assign((size_t)n_filt * d * d, 0.0);
    for (int f = 0; f < n_filt; ++f) {
        double* cf = coef.data() + (size_t)f * n_sec * 5;
        for (int k = 0; k < n_sec; ++k) {
            const double* s = sos + ((size_t)f * n_sec + k) * 6;
            for (int i = 0; i < 6; ++i)
                if (!std::isfinite(s[i])) return false;
            if (s[3] == 0.0) return false;
            const double a0 = s[3];
            cf[5 * k] = s[0] / a0;
            cf[5 * k + 1] = s[1] / a0;
            cf[5 * k + 2] = s[2] / a0;
            cf[5 * k + 3] = s[4] / a0;
            cf[5 * k + 4] = s[5] / a0;
        }
        std::vector<double> a, p, pg;
        carry::sos_transition(cf, n_sec, a);
        carry::carry_powers(a, d, p, pg);
        std::copy(p.begin(), p.end(), phi.begin() + (size_t)f * d * d);
        std::copy(pg.begin(), pg.end(), phig.begin() + (size_t)f * d * d);
    }
    return true;
}

// Everything ds_iir_sos and ds_iir_sos_dev share.  ldx, ld_y: the _dev entry's row strides (the host entry's rows are dense).
struct IirCall {
    const char* who;
    int n_ch;
    int64_t n_samples, ldx, ld_y;
    const double* sos;  // host [n_filt][n_sec][6]
    int n_filt, n_sec, mode;
};

static int iir_check(ds_ctx* c, const IirCall& q, const void* x, const void* y) {
    if (!c || !x || !y || !q.sos) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_ch <= 0 || q.n_samples <= 0 || q.n_filt <= 0 || q.n_sec <= 0 || q.ldx < q.n_samples || q.ld_y < q.n_samples)
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    return DS_OK;
}

// the three passes over device buffers of either sample type; y element (f, c, n) at y[f syf + c syc + n syn]; zi, zf:
// device arrays or nullptr
template <typename T>
static int iir_run(ds_ctx* c, const IirCall& q, const T* x, int64_t sxc, int64_t sxn, const double* zi, T* y, int64_t syf,
                   int64_t syc, int64_t syn, double* zf) {
    if (!fb_mode_ok(q.mode)) return fail(c, DS_ERR_ARG, q.who, "invalid filter bank apply mode");
    // sequential: one cascade of all sections, sos and zi keep their memory layout
    const bool seq = q.mode == DS_FB_SEQUENTIAL;
    const int n_filt = seq ? 1 : q.n_filt, n_sec = seq ? q.n_sec * q.n_filt : q.n_sec, n_ch = q.n_ch;
    if (n_sec > iir::MAX_SEC)
        return fail(c, DS_ERR_UNSUP, q.who, "more than 32 second-order sections in one cascade is not "
                                            "built (the carry's state vector is one value per lane of a wave)");
    CHK(carry_limits(c, q.who, (int64_t)n_filt * n_ch, q.n_samples,
                     "more than 65535 (filter, channel) streams is not built yet"));
    const int64_t n = q.n_samples, n_groups = (n + carry::G - 1) / carry::G;
    std::vector<double> coef, phi, phig;
    if (!iir_tables(q.sos, n_filt, n_sec, coef, phi, phig))
        return fail(c, DS_ERR_ARG, q.who, "sections must be finite with a0 != 0");
    const int d = 2 * n_sec;
    const size_t n_streams = (size_t)n_filt * n_ch;
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, coef.size(), coef.data()}, {8, phi.size(), phi.data()}, {8, phig.size(), phig.data()},
                                        {8, n_streams * n_groups * d}}, t));
    const double *dcoef = (const double*)t[0], *dphi = (const double*)t[1], *dphig = (const double*)t[2];
    double* gst = (double*)t[3];
    iir::Args<T> a{x, sxc, sxn, y, q.mode == DS_FB_PARALLEL ? syf : 0, syc, syn, n, n_ch, n_filt, n_sec,
                   q.mode == DS_FB_SUMMED ? 1 : 0, n_groups, dcoef, dphi, dphig, gst, zi, zf};
    if (n_groups > 1)
        CHK(launch(c, "iir_group", iir::k_iir_group<T>, dim3((unsigned)(n_groups - 1), (unsigned)n_streams), iir::B,
                   iir::lds_bytes(n_sec, false), a));
    carry::CarryArgs ca{dphig, gst, zi, n_groups, n_ch, d};
    CHK(launch(c, "iir_carry", carry::k_block_carry, dim3((unsigned)n_streams), iir::B, sizeof(double) * d * d, ca));
    return launch(c, "iir_apply", iir::k_iir_apply<T>, dim3((unsigned)n_groups, (unsigned)n_ch), iir::B,
                  iir::lds_bytes(n_sec, true), a);
}

extern "C" int ds_iir_sos_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_samples, const double* sos,
                              int n_filt, int n_sec, const double* zi, int mode, float* y, int64_t ld_y, double* zf) {
    const IirCall q{"ds_iir_sos_dev", n_ch, n_samples, ldx, ld_y, sos, n_filt, n_sec, mode};
    CHK(iir_check(c, q, x, y));
    HIPCHK(c, hipSetDevice(c->device));
    return iir_run<float>(c, q, x, ldx, 1, zi, y, (int64_t)n_ch * ld_y, ld_y, 1, zf);
}

// host pointers in the reference's layouts: x (n_samples, n_ch), y (n_filt or 1, n_samples, n_ch), float64; the
// samples cross the link as they are and the kernels read them with the channel stride
extern "C" int ds_iir_sos(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, const double* sos, int n_filt,
                          int n_sec, const double* zi, int mode, double* y, double* zf) {
    const IirCall q{"ds_iir_sos", n_ch, n_samples, n_samples, n_samples, sos, n_filt, n_sec, mode};
    CHK(iir_check(c, q, x, y));
    if (!fb_mode_ok(mode)) return fail(c, DS_ERR_ARG, q.who, "invalid filter bank apply mode");  // it sizes y
    HIPCHK(c, hipSetDevice(c->device));
    const int n_out = mode == DS_FB_PARALLEL ? n_filt : 1;
    const size_t nx = (size_t)n_ch * n_samples, ny = nx * n_out, nz = (size_t)n_filt * n_sec * 2 * n_ch;
    return staged(c, {{8, nx, x}, {8, ny, nullptr, y}, {8, nz, zi}, {8, nz, nullptr, zf}}, [&](void* const* d) {
        return iir_run<double>(c, q, (const double*)d[0], 1, n_ch, zi ? (const double*)d[2] : nullptr, (double*)d[1],
                               (int64_t)nx, 1, n_ch, zf ? (double*)d[3] : nullptr);
    });
}

// ---- IIR filtering with complex coefficients (kernels_ciir.hpp): complex float64 recursion, real samples ------------
typedef std::complex<double> cplx;

// a d x d complex matrix as the kernels read it: the real plane, then the imaginary plane
static void cmat_planes(const std::vector<cplx>& m, int d, double* dst) {
    for (size_t i = 0; i < (size_t)d * d; ++i) {
        dst[i] = m[i].real();
        dst[(size_t)d * d + i] = m[i].imag();
    }
}

// sos [n_filt][n_sec][6] complex -> coef [n_filt][n_sec][5] complex (b0 b1 b2 a1 a2 / a0), phi = A^L, phig = A^(L B),
// each [n_filt][2][D][D]
static bool ciir_tables(const double* sos, int n_filt, int n_sec, std::vector<double>& coef, std::vector<double>& phi,
                        std::vector<double>& phig) {
    const int d = 2 * n_sec;
    coef.assign((size_t)n_filt * n_sec * 10, 0.0);
    phi.assign((size_t)n_filt * 2 * d * d, 0.0);
    phig.assign((size_t)n_filt * 2 * d * d, 0.0);
    for (int f = 0; f < n_filt; ++f) {
        std::vector<cplx> cf((size_t)n_sec * 5);
        for (int k = 0; k < n_sec; ++k) {
            const double* s = sos + ((size_t)f * n_sec + k) * 12;
            for (int i = 0; i < 12; ++i)
                if (!std::isfinite(s[i])) return false;
            const cplx a0(s[6], s[7]);
            if (a0 == cplx(0.0, 0.0)) return false;
            for (int i = 0; i < 5; ++i) {
                const int col = i < 3 ? i : i + 1;
                const cplx v = cplx(s[2 * col], s[2 * col + 1]) / a0;
                cf[5 * k + i] = v;
                coef[((size_t)f * n_sec + k) * 10 + 2 * i] = v.real();
                coef[((size_t)f * n_sec + k) * 10 + 2 * i + 1] = v.imag();
            }
        }
        std::vector<cplx> a, p, pg;
        carry::sos_transition(cf.data(), n_sec, a);
        carry::carry_powers(a, d, p, pg);
        cmat_planes(p, d, phi.data() + (size_t)f * 2 * d * d);
        cmat_planes(pg, d, phig.data() + (size_t)f * 2 * d * d);
    }
    return true;
}

// Everything ds_iir_sos_c128 and a device-pointer caller share.
struct CiirCall {
    const char* who;
    int n_ch;
    int64_t n_samples;
    const double* sos;  // host [n_filt][n_sec][6] complex128
    int n_filt, n_sec;
};

// shape and bounds; nothing touches the device
static int ciir_check(ds_ctx* c, const CiirCall& q, const void* x, const void* yr) {
    if (!c || !x || !yr || !q.sos) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_ch <= 0 || q.n_samples <= 0 || q.n_filt <= 0 || q.n_sec <= 0) return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (q.n_sec > ciir::CIIR_MAX_SEC)
        return fail(c, DS_ERR_UNSUP, q.who, "more than 16 complex second-order sections in one cascade is not built "
                                            "(the carry matrix and the block states of more do not fit the LDS)");
    return carry_limits(c, q.who, (int64_t)q.n_filt * q.n_ch, q.n_samples,
                        "more than 65535 (filter, channel) streams is not built yet");
}

// the tables of a call on the host, and where they and the group states lie on the device
struct CiirTables {
    std::vector<double> coef, phi, phig;
};
struct CiirDev {
    double *coef, *phi, *phig, *gst;
};
static size_t ciir_gst_count(const CiirCall& q) {
    return 2 * (size_t)q.n_filt * q.n_ch * (size_t)((q.n_samples + ciir::G - 1) / ciir::G) * 2 * q.n_sec;
}
static void ciir_take(Carver& cv, const CiirCall& q, CiirDev* dv) {
    const size_t d = 2 * (size_t)q.n_sec;
    dv->coef = cv.take<double>((size_t)q.n_filt * q.n_sec * 10);
    dv->phi = cv.take<double>((size_t)q.n_filt * 2 * d * d);
    dv->phig = cv.take<double>((size_t)q.n_filt * 2 * d * d);
    dv->gst = cv.take<double>(ciir_gst_count(q));
}
static int ciir_upload(ds_ctx* c, const CiirTables& tb, const CiirDev& dv) {
    CHK(ds_upload(c, dv.coef, tb.coef.data(), tb.coef.size() * 8));
    CHK(ds_upload(c, dv.phi, tb.phi.data(), tb.phi.size() * 8));
    return ds_upload(c, dv.phig, tb.phig.data(), tb.phig.size() * 8);
}

// the three passes over device buffers of either sample type; output element (f, c, n) at y?[f syf + c syc + n syn], yi
// may be null; zi, zf: device arrays or nullptr
template <typename T>
static int ciir_run(ds_ctx* c, const CiirCall& q, const CiirDev& dv, const T* x, int64_t sxc, int64_t sxn, const double* zi,
                    double* yr, double* yi, int64_t syf, int64_t syc, int64_t syn, double* zf) {
    const int n_filt = q.n_filt, n_sec = q.n_sec, n_ch = q.n_ch, d = 2 * n_sec;
    const int64_t n = q.n_samples, n_groups = (n + ciir::G - 1) / ciir::G;
    const size_t n_streams = (size_t)n_filt * n_ch;
    ciir::Args<T> a{x, sxc, sxn, yr, yi, syf, syc, syn, n, n_ch, n_filt, n_sec, n_groups, dv.coef, dv.phi, dv.phig, dv.gst, zi, zf};
    if (n_groups > 1)
        CHK(launch(c, "ciir_group", ciir::k_ciir_group<T>, dim3((unsigned)(n_groups - 1), (unsigned)n_streams), ciir::B,
                   ciir::lds_bytes(n_sec, false), a));
    ciir::CarryArgs ca{dv.phig, dv.gst, zi, n_groups, n_ch, n_sec};
    CHK(launch(c, "ciir_carry", ciir::k_ciir_carry, dim3((unsigned)n_streams), ciir::B, sizeof(double) * 2 * d * d, ca));
    return launch(c, "ciir_apply", ciir::k_ciir_apply<T>, dim3((unsigned)n_groups, (unsigned)n_ch), ciir::B,
                  ciir::lds_bytes(n_sec, true), a);
}

// host pointers in the reference's layouts: x (n_samples, n_ch) float64, y_re / y_im (n_filt, n_samples, n_ch) float64
extern "C" int ds_iir_sos_c128(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, const double* sos, int n_filt,
                               int n_sec, const double* zi, double* y_re, double* y_im, double* zf) {
    const CiirCall q{"ds_iir_sos_c128", n_ch, n_samples, sos, n_filt, n_sec};
    CHK(ciir_check(c, q, x, y_re));
    CiirTables tb;
    if (!ciir_tables(sos, n_filt, n_sec, tb.coef, tb.phi, tb.phig))
        return fail(c, DS_ERR_ARG, q.who, "sections must be finite with a0 != 0");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nx = (size_t)n_ch * n_samples, ny = nx * n_filt, nz = (size_t)n_filt * n_sec * 2 * n_ch;
    Carver probe;
    CiirDev dv;
    ciir_take(probe, q, &dv);
    CHK(mem_check(c, q.who, probe.off, 8 * (nx + ny + (y_im ? ny : 0)) + 16 * 2 * nz, 0));
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) { ciir_take(cv, q, &dv); }));
    CHK(ciir_upload(c, tb, dv));
    return staged(c, {{8, nx, x}, {8, ny, nullptr, y_re}, {8, y_im ? ny : 0, nullptr, y_im}, {16, nz, zi}, {16, zf ? nz : 0, nullptr, zf}},
                  [&](void* const* d) {
        return ciir_run<double>(c, q, dv, (const double*)d[0], 1, n_ch, zi ? (const double*)d[3] : nullptr, (double*)d[1],
                                y_im ? (double*)d[2] : nullptr, (int64_t)nx, 1, n_ch, zf ? (double*)d[4] : nullptr);
    });
}

// ---- sums over a pair of signals for distances.snr / si_sdr (kernels_dist.hpp) -----------------------------------
struct PairCall {
    const char* who;
    int n_ch_a, n_ch_b;
    int64_t n;
    int n_ch() const { return std::max(n_ch_a, n_ch_b); }
    int n_wg() const { return (int)((n + dsdist::SPAN - 1) / dsdist::SPAN); }
};

static int pair_check(ds_ctx* c, const PairCall& q, const void* a, const void* b, const void* out) {
    if (!c || !a || !b || !out) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n <= 0 || q.n_ch_a <= 0 || q.n_ch_b <= 0 || (q.n_ch_a != q.n_ch_b && q.n_ch_a != 1 && q.n_ch_b != 1))
        return fail(c, DS_ERR_ARG, q.who, "needs samples, and equal channel counts or one channel on one side");
    if (q.n_ch() > 65535) return fail(c, DS_ERR_UNSUP, q.who, "more than 65535 channels is not built");
    if ((q.n + dsdist::SPAN - 1) / dsdist::SPAN > INT32_MAX) return fail(c, DS_ERR_UNSUP, q.who, "signal too long");
    return DS_OK;
}

// par: host [n_ch][3] or null; out_dev [n_ch][NS]
template <typename T>
static int pair_run(ds_ctx* c, const PairCall& q, const T* a, int64_t sac, int64_t san, const T* b, int64_t sbc, int64_t sbn,
                    const double* par, double* out_dev) {
    const int n_ch = q.n_ch(), n_wg = q.n_wg();
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, par ? (size_t)n_ch * 3 : 0, par}, {8, (size_t)n_ch * n_wg * dsdist::NS}}, t));
    dsdist::PairArgs<T> pa{a, b, q.n_ch_a == 1 ? 0 : sac, san, q.n_ch_b == 1 ? 0 : sbc, sbn, q.n, n_wg,
                           par ? (const double*)t[0] : nullptr, (double*)t[1]};
    CHK(launch(c, "pair_partial", dsdist::k_pair_partial<T>, dim3((unsigned)n_wg, (unsigned)n_ch), dsdist::NT, 0, pa));
    hipLaunchKernelGGL(dsdist::k_pair_final, dim3((unsigned)n_ch), dim3(dsdist::NT), 0, c->stream, (const double*)t[1], n_wg,
                       out_dev);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

// host pointers: a (n, n_ch_a), b (n, n_ch_b) float64; par (n_ch, 3) or NULL; out (n_ch, 6)
extern "C" int ds_pair_moments(ds_ctx* c, const double* a, int n_ch_a, const double* b, int n_ch_b, int64_t n,
                               const double* par, double* out) {
    const PairCall q{"ds_pair_moments", n_ch_a, n_ch_b, n};
    CHK(pair_check(c, q, a, b, out));
    HIPCHK(c, hipSetDevice(c->device));
    return staged(c, {{8, (size_t)n * n_ch_a, a}, {8, (size_t)n * n_ch_b, b}, {8, (size_t)q.n_ch() * dsdist::NS, nullptr, out}},
                  [&](void* const* d) {
        return pair_run<double>(c, q, (const double*)d[0], 1, n_ch_a, (const double*)d[1], 1, n_ch_b, par, (double*)d[2]);
    });
}

// device-resident planar float32 signals, channel ch at a_dev + ch lda
extern "C" int ds_pair_moments_dev(ds_ctx* c, const float* a, int n_ch_a, int64_t lda, const float* b, int n_ch_b, int64_t ldb,
                                   int64_t n, const double* par, double* out) {
    const PairCall q{"ds_pair_moments_dev", n_ch_a, n_ch_b, n};
    CHK(pair_check(c, q, a, b, out));
    if (lda < n || ldb < n) return fail(c, DS_ERR_ARG, q.who, "row stride below the sample count");
    HIPCHK(c, hipSetDevice(c->device));
    return staged(c, {{8, (size_t)q.n_ch() * dsdist::NS, nullptr, out}}, [&](void* const* d) {
        return pair_run<float>(c, q, a, lda, 1, b, ldb, 1, par, (double*)d[0]);
    });
}

// ---- weighted sums of fractionally delayed channels (kernels_delay.hpp) -----------------------------------------
// Everything ds_delay_sum and ds_delay_sum_dev share; the arrays are the host's.
struct DelayCall {
    const char* who;
    int n_src;
    const int64_t* src_len;  // [n_src], each at most n_avail (the samples a source row holds)
    int64_t n_avail;
    int n_rows, n_terms;
    const int* src;          // [n_rows][n_terms], as shift, frac and weight
    const int64_t* shift;
    const double *frac, *weight;
    int order;
    double beta;
    int64_t out_len;
    double* peak;            // [n_rows] or nullptr
    size_t terms() const { return (size_t)n_rows * n_terms; }
};

static int delay_check(ds_ctx* c, const DelayCall& q, const void* x, const void* y) {
    if (!c || !x || (!y && !q.peak) || !q.src_len || !q.src || !q.shift || !q.frac || !q.weight)
        return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_src <= 0 || q.n_rows <= 0 || q.n_terms <= 0 || q.out_len <= 0 || !std::isfinite(q.beta) || q.beta < 0)
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    for (int s = 0; s < q.n_src; ++s)
        if (q.src_len[s] < 0 || q.src_len[s] > q.n_avail) return fail(c, DS_ERR_ARG, q.who, "bad source length");
    if (q.order < 1 || q.order > dly::MAX_ORDER) return fail(c, DS_ERR_UNSUP, q.who, "filter orders 1 to 255 are built");
    // the kernel's window starts and spans are int64 sums of a tile start, a shift and the taps: a quarter of the
    // range leaves them room
    for (size_t e = 0; e < q.terms(); ++e)
        if (q.shift[e] > INT64_MAX / 4 || q.shift[e] < -(INT64_MAX / 4))
            return fail(c, DS_ERR_ARG, q.who, "a term's shift is beyond +-INT64_MAX / 4");
    return DS_OK;
}

// the taps of every term, then the sum; x element (c, n) at x[c sxc + n sxn], y element (g, t) at y[g syg + t syt]
template <typename T>
static int delay_run(ds_ctx* c, const DelayCall& q, const T* x, int64_t sxc, int64_t sxn, T* y, int64_t syg, int64_t syt) {
    const int ntp = (q.order + 1 + dly::R - 1) / dly::R * dly::R, n_rows = q.n_rows;
    const size_t n_t = q.terms();
    if ((n_rows + dly::WAVES - 1) / dly::WAVES > 65535)
        return fail(c, DS_ERR_UNSUP, q.who, "more than 262140 output rows in one call is not built");
    if ((q.out_len + dly::TT - 1) / dly::TT > INT32_MAX || (n_t * ntp + 255) / 256 > (size_t)INT32_MAX)
        return fail(c, DS_ERR_UNSUP, q.who, "output too long or too many terms");
    for (size_t e = 0; e < n_t; ++e)
        if (q.src[e] < 0 || q.src[e] >= q.n_src || !std::isfinite(q.weight[e]) || !(q.frac[e] < 1.0))
            return fail(c, DS_ERR_ARG, q.who, "a term's source, weight or fraction is out of range");
    void* t[kMaxStaged];  // the five tables, the taps of every term, the bits of the peaks
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, (size_t)q.n_src, q.src_len}, {4, n_t, q.src}, {8, n_t, q.shift}, {8, n_t, q.frac},
                                        {8, n_t, q.weight}, {8, n_t * ntp}, {8, q.peak ? (size_t)n_rows : 0}}, t));
    double* dtaps = (double*)t[5];
    unsigned long long* dpk = q.peak ? (unsigned long long*)t[6] : nullptr;
    if (dpk) HIPCHK(c, hipMemsetAsync(dpk, 0, (size_t)n_rows * 8, c->stream));
    dly::TapArgs ta{(const double*)t[3], (int)n_t, q.order, ntp, q.beta, dtaps};
    const int64_t n_tap_threads = (int64_t)n_t * ntp;
    CHK(launch(c, "delay_taps", dly::k_delay_taps, dim3((unsigned)((n_tap_threads + 255) / 256)), 256, 0, ta));
    dly::Args<T> a{x, sxc, sxn, (const int64_t*)t[0], y, syg, syt, q.out_len, n_rows, q.n_terms, ntp, (const int*)t[1],
                   (const int64_t*)t[2], (const double*)t[4], dtaps, dpk};
    CHK(launch(c, "delay_sum", dly::k_delay_sum<T>,
               dim3((unsigned)((q.out_len + dly::TT - 1) / dly::TT), (unsigned)((n_rows + dly::WAVES - 1) / dly::WAVES)),
               dly::THREADS, 0, a));
    if (dpk) CHK(ds_download(c, q.peak, dpk, (size_t)n_rows * 8));  // the bits of non-negative doubles
    return DS_OK;
}

extern "C" int ds_delay_sum_dev(ds_ctx* c, const float* x, int n_src, int64_t ldx, const int64_t* src_len,
                                int n_rows, int n_terms, const int* src, const int64_t* shift, const double* frac,
                                const double* weight, int order, double beta, int64_t out_len, float* y,
                                int64_t ld_y, double* peak) {
    const DelayCall q{"ds_delay_sum_dev", n_src, src_len, ldx, n_rows, n_terms, src, shift, frac, weight, order, beta, out_len, peak};
    CHK(delay_check(c, q, x, y));
    if (y && ld_y < out_len) return fail(c, DS_ERR_ARG, q.who, "bad shape");
    HIPCHK(c, hipSetDevice(c->device));
    return delay_run<float>(c, q, x, ldx, 1, y, ld_y, 1);
}

// host pointers in the reference's layouts: x (n_x, n_src), y (out_len, n_rows), float64
extern "C" int ds_delay_sum(ds_ctx* c, const double* x, int n_src, int64_t n_x, const int64_t* src_len, int n_rows,
                            int n_terms, const int* src, const int64_t* shift, const double* frac,
                            const double* weight, int order, double beta, int64_t out_len, double* y, double* peak) {
    const DelayCall q{"ds_delay_sum", n_src, src_len, n_x, n_rows, n_terms, src, shift, frac, weight, order, beta, out_len, peak};
    CHK(delay_check(c, q, x, y));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nx = (size_t)n_src * n_x, ny = y ? (size_t)n_rows * out_len : 0;
    return staged(c, {{8, nx, x}, {8, ny, nullptr, y}}, [&](void* const* d) {
        return delay_run<double>(c, q, (const double*)d[0], 1, n_src, y ? (double*)d[1] : nullptr, 1, n_rows);
    });
}

// ---- continuous wavelet transform and synchrosqueezing (kernels_cwt.hpp) ---------------------------------------
// Everything ds_cwt and ds_cwt_dev share; the arrays are the host's.
struct CwtCall {
    const char* who;
    int64_t n_samples;
    int n_freq;
    const int64_t* tap_len;        // [n_freq]
    const float2* taps;            // wavelet f's tap_len[f] complex taps at tap_off[f]
    const int* channels;           // [n_ch] planar channels of x to transform
    int n_ch;
    std::vector<int64_t> tap_off;  // set by cwt_check
};

// a, b, out: the entry's own arrays
static int cwt_check(ds_ctx* c, CwtCall& q, const void* a, const void* b, const void* out) {
    if (!c || !a || !b || !out || !q.tap_len || !q.taps) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_samples <= 0 || q.n_freq <= 0) return fail(c, DS_ERR_ARG, q.who, "bad shape");
    q.tap_off.resize(q.n_freq);
    int64_t off = 0;
    for (int f = 0; f < q.n_freq; ++f) {
        if (q.tap_len[f] < 1) return fail(c, DS_ERR_ARG, q.who, "a wavelet has no taps");
        if (q.tap_len[f] > dscwt::MAX_TAPS) return fail(c, DS_ERR_UNSUP, q.who, "wavelets longer than 2^18 taps are not built");
        q.tap_off[f] = off;
        off += q.tap_len[f];
    }
    return DS_OK;
}

// rows f0 .. f0 + n_sel of the scalogram (frequency f0 + i into output row i of out (n_sel, N, n_ch), complex64) of the
// planar fp32 channels q.channels of x
static int cwt_run(ds_ctx* c, const CwtCall& q, const float* x, int64_t ld, int f0, int n_sel, float2* out) {
    using dscwt::Freq;
    const int64_t N = q.n_samples;
    const int n_ch = q.n_ch;
    struct Item { int row; int64_t k0, len, hc; };
    std::map<int, std::vector<Item>> classes;  // by block length M
    for (int i = 0; i < n_sel; ++i) {
        const int64_t L = q.tap_len[f0 + i], h = (L - 1) / 2;
        const int64_t k0 = std::max<int64_t>(0, h - N + 1), k1 = std::min<int64_t>(L - 1, h + N - 1);
        const int64_t lc = k1 - k0 + 1;
        int64_t M = dscwt::MIN_M;
        while (M < 2 * lc) M *= 2;
        classes[(int)M].push_back(Item{i, k0, lc, h - k0});
    }
    for (auto& kv : classes) {
        const int M = kv.first;
        const auto& items = kv.second;
        const int nf = (int)items.size();
        int64_t cc = 0, hmax = 0, ntaps = 0;
        for (const Item& it : items) {
            cc = std::max(cc, it.len - 1 - it.hc);
            hmax = std::max(hmax, it.hc);
        }
        const int64_t V = M - hmax - cc;
        const int64_t nb64 = (N + V - 1) / V;
        if (nb64 > INT32_MAX || nf > 65535 || n_ch > 65535)
            return fail(c, DS_ERR_UNSUP, "cwt: too many blocks, frequencies or channels in one call");
        const int n_blocks = (int)nb64;
        const int64_t n_pairs = (int64_t)n_ch * dscwt::n_block_pairs(n_blocks);  // two blocks of one channel per transform
        std::vector<Freq> fr(nf);
        for (int i = 0; i < nf; ++i) {
            fr[i] = Freq{items[i].row, ntaps, items[i].len, items[i].hc + cc};
            ntaps += items[i].len;
        }
        std::vector<float2> ht((size_t)ntaps);
        for (int i = 0; i < nf; ++i)
            std::memcpy(&ht[fr[i].toff], q.taps + q.tap_off[f0 + items[i].row] + items[i].k0, (size_t)items[i].len * 8);
        const bool big = M > dscwt::MAX_LDS_M;
        const int64_t n_items = (int64_t)nf * n_blocks * n_ch;
        // big route: items per launch pair (the columns stage writes M complex values per item)
        const int64_t chunk = big ? std::min<int64_t>({n_items, 65535, std::max<int64_t>(1, ((int64_t)256 << 20) / (8 * (int64_t)M))}) : 0;
        if (big && n_pairs > 65535)
            return fail(c, DS_ERR_UNSUP, "cwt: more than 65535 four-step block pairs in one call");
        const size_t n_zs = big ? (size_t)std::max<int64_t>({n_pairs, nf, chunk}) * M : 0;
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{4, (size_t)n_ch, q.channels}, {sizeof(Freq), (size_t)nf, fr.data()}, {8, (size_t)ntaps, ht.data()},
                                            {8, (size_t)n_pairs * M}, {8, (size_t)nf * M}, {8, n_zs}}, t));
        const int* dch = (const int*)t[0];
        const Freq* dfr = (const Freq*)t[1];
        const float2* dtaps = (const float2*)t[2];
        float2 *Z = (float2*)t[3], *W = (float2*)t[4], *zs = (float2*)t[5];
        const float inv_m = 1.0f / (float)M;
        if (!big) {
            const float2* tw;
            CHK(get_twiddles(c, M, &tw));
            dscwt::WspecArgs wa{dtaps, dfr, inv_m, W, tw};
            dscwt::FwdArgs fa{x, ld, N, dch, n_ch, n_blocks, V, cc, Z, tw};
            dscwt::InvArgs ia{Z, W, dfr, n_ch, n_blocks, V, N, out, tw};
            const int rc = dispatch<256, 512, 1024, 2048, 4096, 8192, 16384>(M, [&](auto k) {
                constexpr int NN = decltype(k)::value;
                const size_t lds = Plan<NN>::LDS_BYTES;
                CHK(launch(c, "cwt_wspec", dscwt::k_cwt_wspec<NN>, dim3(nf), Plan<NN>::NT, lds, wa));
                CHK(launch(c, "cwt_fwd", dscwt::k_cwt_fwd<NN>, dim3(dscwt::n_block_pairs(n_blocks), n_ch), Plan<NN>::NT, lds, fa));
                return launch(c, "cwt_inv", dscwt::k_cwt_inv<NN>, dim3(n_blocks, n_ch, nf), Plan<NN>::NT, lds, ia);
            });
            if (rc != DS_OK) return rc;
            continue;
        }
        // four-step route: tap spectra and block spectra through the bigfft stages, then the fused inverse
        const int grid_x = (int)std::min<int64_t>(1024, (M + 255) / 256);
        CHK(launch(c, "cwt_pad@big", dscwt::k_cwt_pad, dim3(grid_x, nf), 256, 0, dscwt::PadArgs{dtaps, dfr, M, inv_m, zs}));
        CHK(big_cols(c, zs, nullptr, 0, 0, 0, zs, M, nf));
        CHK(big_rows(c, zs, W, M, nf));
        CHK(launch(c, "cwt_segments@big", dscwt::k_cwt_segments, dim3(grid_x, (unsigned)n_pairs), 256, 0,
                   dscwt::SegArgs{x, ld, N, dch, n_ch, n_blocks, V, cc, M, zs}));
        CHK(big_cols(c, zs, nullptr, 0, 0, 0, zs, M, (int)n_pairs));
        CHK(big_rows(c, zs, Z, M, (int)n_pairs));
        constexpr int N1 = dscwt::BIG_N1;
        const int n2 = M / N1;
        const float2 *tw1, *tw2;
        CHK(get_twiddles(c, N1, &tw1));
        CHK(get_twiddles(c, n2, &tw2));
        const int ct1 = std::min(8, n2), ct2 = big_rows_ct(n2);
        for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
            const unsigned cnt = (unsigned)std::min<int64_t>(chunk, n_items - i0);
            dscwt::BigInvArgs a{Z, W, dfr, n_ch, n_blocks, i0, M, V, N, n2, ct1, zs, out, tw1};
            CHK(launch(c, "cwt_bcols@big", dscwt::k_cwt_bcols<N1>, dim3(n2 / ct1, cnt), ct1 * Cfg<N1>::NT,
                       (size_t)ct1 * dsbig::ch_stride<N1>() * sizeof(float2), a));
            a.ct = ct2;
            a.tw = tw2;
            const int rc = dispatch<32, 64, 128, 256, 512>(n2, [&](auto k) {
                constexpr int NN = decltype(k)::value;
                return launch(c, "cwt_brows@big", dscwt::k_cwt_brows<NN>, dim3(N1 / ct2, cnt), ct2 * Cfg<NN>::NT,
                              (size_t)ct2 * dsbig::ch_stride<NN>() * sizeof(float2), a);
            });
            if (rc != DS_OK) return rc;
        }
    }
    return DS_OK;
}

extern "C" int ds_cwt_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_samples, const int* channels,
                          int n_out_ch, int n_freq, const int64_t* tap_len, const float* taps, float* out) {
    CwtCall q{"ds_cwt_dev", n_samples, n_freq, tap_len, (const float2*)taps, channels, n_out_ch};
    CHK(cwt_check(c, q, x, channels, out));
    if (n_ch <= 0 || n_out_ch <= 0 || ldx < n_samples) return fail(c, DS_ERR_ARG, "ds_cwt_dev: bad shape");
    for (int i = 0; i < n_out_ch; ++i)
        if (channels[i] < 0 || channels[i] >= n_ch) return fail(c, DS_ERR_ARG, "ds_cwt_dev: channel out of range");
    HIPCHK(c, hipSetDevice(c->device));
    return cwt_run(c, q, x, ldx, 0, n_freq, (float2*)out);
}

// host: x (n_samples, n_ch) float64, out (n_freq, n_samples, n_ch) complex64 (out_f64 = 0) or complex128; the
// scalogram is computed in frequency chunks of at most 512 MB of complex64 on the device, so this entry places and
// copies its two arrays itself instead of going through staged()
extern "C" int ds_cwt(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, int n_freq, const int64_t* tap_len,
                      const float* taps, int out_f64, void* out) {
    CwtCall q{"ds_cwt", n_samples, n_freq, tap_len, (const float2*)taps, nullptr, n_ch};
    CHK(cwt_check(c, q, x, x, out));
    if (n_ch <= 0) return fail(c, DS_ERR_ARG, "ds_cwt: bad shape");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t row = n_samples * n_ch;  // complex values per frequency
    const int rows = (int)std::max<int64_t>(1, std::min<int64_t>(n_freq, ((int64_t)512 << 20) / (8 * row)));
    float* dx;
    float2* dout;
    CHK(carve(c, &c->io, &c->io_bytes, [&](Carver& cv) {
        dx = cv.take<float>((size_t)n_ch * n_samples);
        dout = cv.take<float2>((size_t)rows * row);
    }));
    CHK(upload_signal(c, nullptr, x, n_samples, n_ch, dx));
    std::vector<int> ch(n_ch);
    for (int i = 0; i < n_ch; ++i) ch[i] = i;
    q.channels = ch.data();
    for (int f0 = 0; f0 < n_freq; f0 += rows) {
        const int nr = std::min(rows, n_freq - f0);
        CHK(cwt_run(c, q, dx, n_samples, f0, nr, dout));
        if (out_f64)
            CHK(download_widen(c, (const float*)dout, 2 * nr * row, (double*)out + 2 * f0 * row));
        else
            CHK(ds_download(c, (float*)out + 2 * f0 * row, dout, (size_t)nr * row * 8));
    }
    return DS_OK;
}

extern "C" int ds_cwt_squeeze_dev(ds_ctx* c, const float* s, int n_freq, int64_t n_samples, int n_ch,
                                  const double* freqs, const double* delta_f, const double* norm, double fs,
                                  double* out) {
    if (!c || !s || !freqs || !delta_f || !out) return fail(c, DS_ERR_ARG, "ds_cwt_squeeze_dev: null argument");
    if (n_freq <= 0 || n_ch <= 0 || n_samples < 2)
        return fail(c, DS_ERR_ARG, "ds_cwt_squeeze_dev: bad shape (the gradient needs two samples)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nf = (size_t)n_freq;
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, nf, freqs}, {8, nf, delta_f}, {8, norm ? nf : 0, norm}}, t));
    const int64_t cols = n_samples * n_ch;
    dscwt::SqueezeArgs a{(const float2*)s, n_freq, n_ch, n_samples, (const double*)t[0], (const double*)t[1],
                         norm ? (const double*)t[2] : nullptr, fs, (double2*)out};
    return launch(c, "cwt_squeeze", dscwt::k_cwt_squeeze, dim3((unsigned)((cols + 255) / 256)), 256, 0, a);
}

// ---- fractional-octave smoothing (kernels_smooth.hpp), float64 -----------------------------------------------
// what both entries refuse (n_ch: real columns); then wr: the window reversed and normalised by its sum, as the kernel
// reads it
static int smooth_check(ds_ctx* c, const char* who, int64_t n_bins, int n_ch, const double* k_log, const double* window,
                        int64_t n_window, std::vector<double>& wr) {
    if (n_bins < 1 || n_ch < 1 || n_window < 1 || (int64_t)n_ch * 2 > INT32_MAX / 2)
        return fail(c, DS_ERR_ARG, who, "bad shape");
    if (k_log) {
        // k_to_lin brackets every linear bin 1 .. N between two points of k_log: no extrapolation, as in the reference
        if (n_bins < 2) return fail(c, DS_ERR_ARG, who, "the logarithmic axis needs two bins");
        if (!(k_log[0] <= 1.0) || !(k_log[n_bins - 1] >= (double)n_bins))
            return fail(c, DS_ERR_ARG, who, "k_log does not span the bins 1 .. n_bins");
        for (int64_t i = 1; i < n_bins; ++i)
            if (!(k_log[i] > k_log[i - 1])) return fail(c, DS_ERR_ARG, who, "k_log is not strictly ascending");
    }
    double sum = 0.0;
    for (int64_t k = 0; k < n_window; ++k) sum += window[k];
    if (!(std::fabs(sum) > 0.0) || !std::isfinite(sum)) return fail(c, DS_ERR_ARG, who, "the window sums to zero");
    if (smooth_work_too_large(n_bins, n_window, n_ch))
        return fail(c, DS_ERR_UNSUP, who, "bins x window x channels is beyond the direct summation's work bound");
    if ((n_bins * n_ch + dssmooth::NT - 1) / dssmooth::NT > INT32_MAX)
        return fail(c, DS_ERR_UNSUP, who, "more values than one launch covers");
    wr.assign(n_window, 0.0);
    for (int64_t k = 0; k < n_window; ++k) wr[k] = window[n_window - 1 - k] / sum;
    return DS_OK;
}

// the three real passes on a dense device array v (n_bins, n_ch); the result lands in `out`, a and b are two more
// arrays of that size.  klog / wr: device copies of k_log (or nullptr) and of the reversed window.
static int smooth_run(ds_ctx* c, const double* v, int64_t n_bins, int n_ch, const double* klog, const double* wr,
                      int64_t n_window, int clip_ch, double* a, double* b, double* out) {
    using namespace dssmooth;
    const dim3 flat((unsigned)((n_bins * n_ch + NT - 1) / NT));
    int tc = 1, lg = 0;
    while (tc < MAX_TC && tc < n_ch) tc <<= 1, ++lg;
    const dim3 tiles((unsigned)((n_bins + smooth_tile_bins(tc) - 1) / smooth_tile_bins(tc)), (unsigned)((n_ch + tc - 1) / tc));
    if (!klog) {
        CHK(launch(c, "smooth", k_smooth, tiles, NT, 0, SmoothArgs{v, wr, n_bins, n_window, n_ch, tc, lg, out}));
        if (clip_ch > 0) CHK(launch(c, "smooth_clip", k_clip, flat, NT, 0, ClipArgs{out, n_bins, n_ch, clip_ch}));
        return DS_OK;
    }
    CHK(launch(c, "smooth_to_log", k_to_log, flat, NT, 0, LogArgs{v, klog, n_bins, n_ch, a}));
    CHK(launch(c, "smooth", k_smooth, tiles, NT, 0, SmoothArgs{a, wr, n_bins, n_window, n_ch, tc, lg, b}));
    return launch(c, "smooth_to_lin", k_to_lin, flat, NT, 0,
                  LinArgs{b, klog, n_bins, n_ch, clip_ch, (double)(n_bins - 1) / std::log((double)n_bins), out});
}

extern "C" int ds_octave_smooth(ds_ctx* c, const double* v, int64_t n_bins, int n_ch, const double* k_log,
                                const double* window, int64_t n_window, int clip, double* out) {
    if (!c || !v || !window || !out) return fail(c, DS_ERR_ARG, "ds_octave_smooth: null argument");
    std::vector<double> wr;
    CHK(smooth_check(c, "ds_octave_smooth", n_bins, n_ch, k_log, window, n_window, wr));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_bins * n_ch, nl = k_log ? n : 0;
    void* t[kMaxStaged];  // the two arrays between the passes, k_log, the window
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, nl}, {8, nl}, {8, k_log ? (size_t)n_bins : 0, k_log}, {8, wr.size(), wr.data()}}, t));
    return staged(c, {{8, n, v}, {8, n, nullptr, out}}, [&](void* const* d) {
        return smooth_run(c, (const double*)d[0], n_bins, n_ch, k_log ? (const double*)t[2] : nullptr, (const double*)t[3],
                          n_window, clip ? n_ch : 0, (double*)t[0], (double*)t[1], (double*)d[1]);
    });
}

// z, out: (n_bins, n_ch) complex128.  |z| and the unwrapped phase are smoothed as the 2 n_ch columns of one real array
// and recombined; everything between the upload of z and the download of the result stays on the device.
extern "C" int ds_octave_smooth_complex(ds_ctx* c, const double* z, int64_t n_bins, int n_ch, const double* k_log,
                                        const double* window, int64_t n_window, int clip_magnitude, double* out) {
    using namespace dssmooth;
    if (!c || !z || !window || !out) return fail(c, DS_ERR_ARG, "ds_octave_smooth_complex: null argument");
    std::vector<double> wr;
    CHK(smooth_check(c, "ds_octave_smooth_complex", n_bins, 2 * n_ch, k_log, window, n_window, wr));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_bins * n_ch, nl = k_log ? 2 * n : 0;
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, 2 * n},  // (its magnitude columns stay unused) | wrapped phase
                                        {8, 2 * n},  // magnitude | unwrapped phase
                                        {8, nl}, {8, nl}, {8, 2 * n},  // between the passes; the smoothed columns
                                        {8, k_log ? (size_t)n_bins : 0, k_log}, {8, wr.size(), wr.data()}}, t));
    double *dmp = (double*)t[0], *dun = (double*)t[1], *dsm = (double*)t[4];
    return staged(c, {{16, n, z, out}}, [&](void* const* d) {  // the spectrum, then the result
        double2* dz = (double2*)d[0];
        const dim3 flat((unsigned)((n + NT - 1) / NT));
        CHK(launch(c, "smooth_polar", k_polar, flat, NT, 0, PolarArgs{dz, n_bins, n_ch, dun, dmp}));
        CHK(launch(c, "smooth_unwrap", k_unwrap, dim3((unsigned)n_ch), NT, 0,
                   UnwrapArgs{dmp + n_ch, n_bins, 2 * (int64_t)n_ch, dun + n_ch}));
        CHK(smooth_run(c, dun, n_bins, 2 * n_ch, k_log ? (const double*)t[5] : nullptr, (const double*)t[6], n_window,
                       clip_magnitude ? n_ch : 0, (double*)t[2], (double*)t[3], dsm));
        return launch(c, "smooth_recombine", k_recombine, flat, NT, 0, RecombineArgs{dsm, n_bins, n_ch, dz});
    });
}

// ---- direct sums (kernels_direct.hpp), float64 --------------------------------------------------------------
// Everything ds_dft and ds_dft_dev share.  x: device samples, element (n, c) at x[n ss + c cs]; out: the device's copy
// of q.out.
struct DftCall {
    const char* who;
    int64_t n_samples;
    int n_ch;
    const double* freqs_hz;
    int64_t n_freq;
    double fs;
    const double* alpha;  // nullptr: the plain DFT
    const int64_t* peak;
    double half, min_weight_log2;
    double* out;          // host (n_freq, n_ch) complex128
};

// validation, the kept distances of the windowed form and the work bound; nothing touches the device.  *empty: the
// result has no elements.
static int dft_check(ds_ctx* c, const DftCall& q, std::vector<int64_t>& dist, bool* empty) {
    *empty = q.n_freq == 0 || q.n_ch == 0;
    if (q.n_freq < 0 || q.n_ch < 0 || q.n_samples < 1 || !(q.fs > 0.0)) return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (*empty) return DS_OK;
    const double N = (double)q.n_samples, C = (double)q.n_ch;
    // an upper bound first: it needs no array, and a frequency count beyond it is never walked
    if (!q.alpha && dft_work_too_large((double)q.n_freq * N * C, false))
        return fail(c, DS_ERR_UNSUP, q.who, "frequencies x samples x channels is beyond the direct summation's work bound");
    if ((q.n_freq + dsdirect::FT - 1) / dsdirect::FT > INT32_MAX || (q.n_ch + dsdirect::CT - 1) / dsdirect::CT > 65535 ||
        q.n_freq * q.n_ch > INT64_MAX / 64)
        return fail(c, DS_ERR_UNSUP, q.who, "more frequencies or channels than one launch covers");
    if (!q.freqs_hz || !q.out) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (!q.alpha) return DS_OK;
    // every (bin, channel) keeps its peak sample at least
    if (dft_work_too_large((double)q.n_freq * C, true) || q.n_freq > ((int64_t)1 << 28))
        return fail(c, DS_ERR_UNSUP, q.who, "the kept window terms are beyond the direct summation's work bound");
    if (!q.peak || !(q.half > 0.0) || std::isnan(q.min_weight_log2) || q.min_weight_log2 > 0.0)
        return fail(c, DS_ERR_ARG, q.who, "the windowed form needs peak, half > 0 and min_weight_log2 <= 0");
    for (int ch = 0; ch < q.n_ch; ++ch)
        if (q.peak[ch] < 0 || q.peak[ch] >= q.n_samples) return fail(c, DS_ERR_ARG, q.who, "peak outside the signal");
    // weight(d) = exp(-alpha (d / half)^2 / 2) >= 2^min_weight_log2  <=>  d <= half sqrt(-2 ln2 min_weight_log2 / alpha)
    dist.resize(q.n_freq);
    double terms = 0.0;
    for (int64_t k = 0; k < q.n_freq; ++k) {
        const double a = q.alpha[k];
        if (std::isnan(a)) return fail(c, DS_ERR_ARG, q.who, "alpha is NaN");
        const double d = a > 0.0 ? q.half * std::sqrt(-2.0 * 0.6931471805599453 * q.min_weight_log2 / a) : N;
        dist[k] = d < N ? (int64_t)d : q.n_samples;
        for (int ch = 0; ch < q.n_ch; ++ch)
            terms += (double)(std::min(q.n_samples, q.peak[ch] + dist[k] + 1) - std::max<int64_t>(0, q.peak[ch] - dist[k]));
    }
    if (dft_work_too_large(terms, true))
        return fail(c, DS_ERR_UNSUP, q.who, "the kept window terms are beyond the direct summation's work bound");
    return DS_OK;
}

template <typename T>
static int dft_run(ds_ctx* c, const DftCall& q, const T* x, int64_t ss, int64_t cs, const std::vector<int64_t>& dist,
                   double2* out) {
    using namespace dsdirect;
    const int64_t F = q.n_freq, n_out = F * q.n_ch;
    const int64_t ftiles = (F + FT - 1) / FT, ctiles = (q.n_ch + CT - 1) / CT;
    // sample chunks: enough workgroups to fill the device when the frequencies alone do not
    const int64_t units = (q.n_samples + CHUNK_UNIT - 1) / CHUNK_UNIT;
    const int64_t want = std::max<int64_t>(1, 4096 / (ftiles * ctiles));
    const int64_t chunk = (units + std::min(units, want) - 1) / std::min(units, want) * CHUNK_UNIT;
    const int n_chunks = (int)((q.n_samples + chunk - 1) / chunk);
    const size_t nw = q.alpha ? (size_t)F : 0;  // the windowed form's three tables
    void* t[kMaxStaged];  // frequencies, alpha, kept distances, peaks, the chunks' partial sums
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, (size_t)F, q.freqs_hz}, {8, nw, q.alpha}, {8, nw, dist.data()},
                                        {8, q.alpha ? (size_t)q.n_ch : 0, q.peak}, {16, (size_t)n_chunks * n_out}}, t));
    double2* dpart = (double2*)t[4];
    DftArgs a{x, ss, cs, q.n_samples, q.n_ch, (const double*)t[0], F, q.fs, (const double*)t[1], (const int64_t*)t[3],
              (const int64_t*)t[2], q.half, chunk, dpart};
    const dim3 grid((unsigned)ftiles, (unsigned)n_chunks, (unsigned)ctiles);
    if (q.alpha)
        CHK(launch(c, "dft@windowed", k_dft<T, true>, grid, NT, 0, a));
    else
        CHK(launch(c, "dft", k_dft<T, false>, grid, NT, 0, a));
    return launch(c, "dft_combine", k_dft_combine, dim3((unsigned)((n_out + NT - 1) / NT)), NT, 0,
                  CombineArgs{dpart, n_out, n_chunks, out});
}

extern "C" int ds_dft(ds_ctx* c, const double* x, int64_t n_samples, int n_ch, const double* freqs_hz, int64_t n_freq,
                      double fs_hz, const double* alpha, const int64_t* peak, double half, double min_weight_log2,
                      double* out) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_dft: null context");
    const DftCall q{"ds_dft", n_samples, n_ch, freqs_hz, n_freq, fs_hz, alpha, peak, half, min_weight_log2, out};
    std::vector<int64_t> dist;
    bool empty;
    CHK(dft_check(c, q, dist, &empty));
    if (empty) return DS_OK;
    if (!x) return fail(c, DS_ERR_ARG, "ds_dft: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    return staged(c, {{8, (size_t)n_samples * n_ch, x}, {16, (size_t)n_freq * n_ch, nullptr, out}}, [&](void* const* d) {
        return dft_run<double>(c, q, (const double*)d[0], n_ch, 1, dist, (double2*)d[1]);
    });
}

extern "C" int ds_dft_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_samples, const double* freqs_hz,
                          int64_t n_freq, double fs_hz, const double* alpha, const int64_t* peak, double half,
                          double min_weight_log2, double* out) {
    if (!c) return fail(c, DS_ERR_ARG, "ds_dft_dev: null context");
    const DftCall q{"ds_dft_dev", n_samples, n_ch, freqs_hz, n_freq, fs_hz, alpha, peak, half, min_weight_log2, out};
    std::vector<int64_t> dist;
    bool empty;
    CHK(dft_check(c, q, dist, &empty));
    if (empty) return DS_OK;
    if (!x || ldx < n_samples) return fail(c, DS_ERR_ARG, "ds_dft_dev: null samples or ldx < n_samples");
    HIPCHK(c, hipSetDevice(c->device));
    return staged(c, {{16, (size_t)n_freq * n_ch, nullptr, out}}, [&](void* const* d) {
        return dft_run<float>(c, q, x, 1, ldx, dist, (double2*)d[0]);
    });
}

// z, out: host (n_bins, n_ch) complex128.  ind_low / ind_high: the band of every bin clipped to [0, n_bins];
// window_length: its unclipped length; pass: bins copied unchanged.  domain: DS_SMOOTH_* of the header.
extern "C" int ds_complex_smooth(ds_ctx* c, const double* z, int64_t n_bins, int n_ch, const int32_t* ind_low,
                                 const int32_t* ind_high, const int32_t* window_length, const int32_t* pass,
                                 const double* window_x, const double* window_y, int n_window, int domain, double* out) {
    using namespace dsdirect;
    if (!c) return fail(c, DS_ERR_ARG, "ds_complex_smooth: null context");
    if (n_bins < 0 || n_ch < 0 || n_bins > INT32_MAX / 2 || n_ch > INT32_MAX / 4 || n_window < 2)
        return fail(c, DS_ERR_ARG, "ds_complex_smooth: bad shape");
    if (domain < DS_SMOOTH_REAL_IMAGINARY || domain > DS_SMOOTH_EQUIVALENT_COMPLEX)
        return fail(c, DS_ERR_ARG, "ds_complex_smooth: unknown domain");
    if (n_bins == 0 || n_ch == 0) return DS_OK;
    if (!z || !ind_low || !ind_high || !window_length || !pass || !window_x || !window_y || !out)
        return fail(c, DS_ERR_ARG, "ds_complex_smooth: null argument");
    double terms = 0.0;
    for (int64_t i = 0; i < n_bins; ++i) {
        if (pass[i]) continue;
        if (ind_low[i] < 0 || ind_high[i] > n_bins || ind_low[i] >= ind_high[i] ||
            window_length[i] < ind_high[i] - ind_low[i])
            return fail(c, DS_ERR_ARG, "ds_complex_smooth: a band leaves the spectrum or its window");
        terms += (double)(ind_high[i] - ind_low[i]);
    }
    if (csmooth_work_too_large(terms * (double)n_ch))
        return fail(c, DS_ERR_UNSUP, "ds_complex_smooth: band lengths x channels is beyond the direct summation's work bound");
    for (int k = 1; k < n_window; ++k)
        if (!(window_x[k] > window_x[k - 1])) return fail(c, DS_ERR_ARG, "ds_complex_smooth: window_x is not ascending");
    if ((n_bins + WAVES - 1) / WAVES > INT32_MAX || (2 * (int64_t)n_ch + WCT - 1) / WCT > 65535)
        return fail(c, DS_ERR_UNSUP, "ds_complex_smooth: more bins or channels than one launch covers");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_bins * n_ch;
    const int64_t ld = 2 * (int64_t)n_ch;
    const size_t nb = (size_t)n_bins, nw = (size_t)n_window;
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, 2 * n},  // the domain's quantity: (bins, 2 C) real columns
                                        {8, 2 * n},  // wrapped phases, values nobody reads
                                        {8, 2 * n},  // smoothed columns
                                        {8, nw, window_x}, {8, nw, window_y}, {4, nb, ind_low}, {4, nb, ind_high},
                                        {4, nb, window_length}, {4, nb, pass}}, t));
    double *da = (double*)t[0], *db = (double*)t[1], *ds = (double*)t[2];
    return staged(c, {{16, n, z}, {16, n, nullptr, out}}, [&](void* const* d) {
        const double* dz = (const double*)d[0];
        double* dres = (double*)d[1];
        const dim3 flat((unsigned)((n + NT - 1) / NT));
        // the band sums of the leading n_cols columns of a (bins, 2 C) array
        auto smooth = [&](const double* v, double* o, int n_cols) {
            return launch(c, "csmooth", k_csmooth, dim3((unsigned)((n_bins + WAVES - 1) / WAVES), (unsigned)((n_cols + WCT - 1) / WCT)),
                          NT, 0, CsmoothArgs{v, ld, o, ld, n_cols, n_bins, (const int*)t[5], (const int*)t[6], (const int*)t[7],
                                             (const int*)t[8], (const double*)t[3], (const double*)t[4], n_window});
        };
        auto polar = [&](const double* zz, double* mag, double* ph) {
            return launch(c, "csmooth_polar", dssmooth::k_polar, flat, NT, 0,
                          dssmooth::PolarArgs{(const double2*)zz, n_bins, n_ch, mag, ph});
        };
        auto colmap = [&](double* v, int root) {
            return launch(c, "csmooth_map", k_colmap, flat, NT, 0, ColmapArgs{v, n_bins, ld, n_ch, root});
        };
        const bool power = domain == DS_SMOOTH_POWER_PHASE || domain == DS_SMOOTH_POWER || domain == DS_SMOOTH_EQUIVALENT_COMPLEX;
        switch (domain) {
        case DS_SMOOTH_REAL_IMAGINARY:  // (re, im) interleaved are 2 C real columns as they stand
            return smooth(dz, dres, 2 * n_ch);
        case DS_SMOOTH_MAGNITUDE_PHASE:
        case DS_SMOOTH_POWER_PHASE:  // da = magnitude or power | unwrapped phase, all smoothed
            CHK(polar(dz, da, db));
            CHK(launch(c, "csmooth_unwrap", dssmooth::k_unwrap, dim3((unsigned)n_ch), NT, 0,
                       dssmooth::UnwrapArgs{db + n_ch, n_bins, ld, da + n_ch}));
            if (power) CHK(colmap(da, 0));
            CHK(smooth(da, ds, 2 * n_ch));
            break;
        case DS_SMOOTH_MAGNITUDE:
        case DS_SMOOTH_POWER:  // the phase of the input goes straight into ds; only the magnitudes are smoothed
            CHK(polar(dz, da, ds));
            if (power) CHK(colmap(da, 0));
            CHK(smooth(da, ds, n_ch));
            break;
        default:  // DS_SMOOTH_EQUIVALENT_COMPLEX: the phase of the smoothed spectrum, the smoothed power
            CHK(smooth(dz, da, 2 * n_ch));
            CHK(polar(da, db, ds));
            CHK(polar(dz, da, db));
            CHK(colmap(da, 0));
            CHK(smooth(da, ds, n_ch));
        }
        if (power) CHK(colmap(ds, 1));
        return launch(c, "csmooth_recombine", dssmooth::k_recombine, flat, NT, 0,
                      dssmooth::RecombineArgs{ds, n_bins, n_ch, (double2*)dres});
    });
}

// ---- complex128 transforms of any length and what is built on them (kernels_fft64.hpp) -----------------------------
struct Fft64Plan {
    int64_t n = 0, ld = 0;  // ld: the column stride on the device, n or Bluestein's M
    int lg = 0;             // log2 of the power-of-two transform that runs (of n or of M)
    bool blue = false;
    const double2 *tw = nullptr, *w = nullptr, *B = nullptr;
};
static const size_t kBlue64CapBytes = (size_t)256 << 20;

// the power-of-two transform of n_cols columns, unnormalised; the result is in x afterwards (x and tmp may have swapped)
static int fft64_pow2(ds_ctx* c, const double2* tw, double2*& x, double2*& tmp, int64_t n, int lg, int n_cols,
                      int64_t col_stride, bool inv) {
    using namespace fft64;
    auto lds = [&](double2* buf, int len, int lgl, int64_t batches, int64_t twid_n) {
        const LdsArgs a{buf, col_stride, len, lgl, tw, twid_n};
        const dim3 grid((unsigned)batches, (unsigned)n_cols);
        return inv ? launch(c, "fft64_lds@inv", k_fft_lds<true>, grid, NT, (size_t)len * 16, a)
                   : launch(c, "fft64_lds", k_fft_lds<false>, grid, NT, (size_t)len * 16, a);
    };
    if (n <= LDS_MAX) return n > 1 ? lds(x, (int)n, lg, 1, 0) : DS_OK;
    const int lg1 = lg / 2, lg2 = lg - lg1, n1 = 1 << lg1, n2 = 1 << lg2;  // x[j1 n2 + j2]
    auto transpose = [&](const double2* in, double2* out, int rows, int cols) {
        return launch(c, "fft64_transpose", k_transpose, dim3((unsigned)(cols / 32), (unsigned)(rows / 32), (unsigned)n_cols), NT, 0,
                      TransposeArgs{in, out, rows, cols, col_stride});
    };
    CHK(transpose(x, tmp, n1, n2));  // [j2][j1]
    CHK(lds(tmp, n1, lg1, n2, n));   // [j2][k1] w_n^(j2 k1)
    CHK(transpose(tmp, x, n2, n1));  // [k1][j2]
    CHK(lds(x, n2, lg2, n1, 0));     // [k1][k2]
    CHK(transpose(x, tmp, n1, n2));  // [k2][k1]: bin k1 + n1 k2
    std::swap(x, tmp);
    return DS_OK;
}

// Bluestein's tables of length n: built once, kept until the cap pushes the least recently used ones out
static int fft64_blue_tables(ds_ctx* c, Fft64Plan* pl) {
    using namespace fft64;
    const int64_t n = pl->n, M = pl->ld;
    auto it = c->blue64.find(n);
    if (it == c->blue64.end()) {
        const size_t bytes = (size_t)(n + M) * 16;
        while (!c->blue64.empty() && c->blue64_bytes + bytes > kBlue64CapBytes) {
            auto old = c->blue64.begin();
            for (auto e = c->blue64.begin(); e != c->blue64.end(); ++e)
                if (e->second.stamp < old->second.stamp) old = e;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipFree(old->second.ptr));
            c->blue64_bytes -= old->second.bytes;
            c->blue64.erase(old);
        }
        double2* tmp;
        CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) { tmp = cv.take<double2>(M); }));
        double2* tab;
        if (hipMalloc((void**)&tab, bytes) != hipSuccess) return fail(c, DS_ERR_NOMEM, "fft64: hipMalloc of the chirp tables failed");
        double2* B = tab + n;
        int rc = launch(c, "fft64_chirp", k_chirp, dim3((unsigned)((M + NT - 1) / NT)), NT, 0, ChirpArgs{tab, B, n, M});
        double2* res = B;
        if (rc == DS_OK) rc = fft64_pow2(c, pl->tw, res, tmp, M, pl->lg, 1, M, false);
        if (rc == DS_OK && res != B && hipMemcpyAsync(B, res, (size_t)M * 16, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            rc = fail(c, DS_ERR_HIP, "fft64: copy of the chirp spectrum failed");
        if (rc != DS_OK) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(tab);
            return rc;
        }
        it = c->blue64.emplace(n, ds_ctx::Blue64Entry{tab, bytes, 0}).first;
        c->blue64_bytes += bytes;
    }
    it->second.stamp = ++c->blue_clock;
    pl->w = it->second.ptr;
    pl->B = it->second.ptr + n;
    return DS_OK;
}

// What every entry checks before anything is uploaded: the shape, the two length bounds, the device memory the call
// will hold (mem_check: two planar buffers, `extra` bytes of further workspace, `io` bytes of staging, the tables); then
// the tables.
// The entry carves its workspace next, still before staged() uploads anything.
static int fft64_plan(ds_ctx* c, const char* who, int64_t n, int64_t n_ch, size_t extra, size_t io, Fft64Plan* pl) {
    if (n < 1 || n_ch < 1) return fail(c, DS_ERR_ARG, who, "bad shape");
    if (fft64_len_unsupported(n))
        return fail(c, DS_ERR_UNSUP, who, "transform lengths above 2^22 (powers of two) or 2^21 (any other) are not built");
    if (n_ch > 65535) return fail(c, DS_ERR_UNSUP, who, "more than 65535 channels in one call is not built");
    pl->n = n;
    pl->blue = !is_pow2(n);
    int64_t M = 1;
    int lg = 0;
    while (M < (pl->blue ? 2 * n - 1 : n)) M <<= 1, ++lg;
    pl->ld = M;
    pl->lg = lg;
    const bool have_tab = pl->blue && c->blue64.count(n);
    CHK(mem_check(c, who, 2 * (size_t)M * (size_t)n_ch * 16 + extra, io, pl->blue && !have_tab ? (size_t)(n + 2 * M) * 16 : 0));
    if (!c->fft64_tw) {
        HIPCHK(c, hipMalloc((void**)&c->fft64_tw, (size_t)(fft64::LDS_MAX / 2) * 16));
        hipLaunchKernelGGL(f64c::k_twiddles, dim3(fft64::LDS_MAX / 2 / 256), dim3(256), 0, c->stream, c->fft64_tw, fft64::LDS_MAX / 2);
        HIPCHK(c, hipGetLastError());
    }
    pl->tw = c->fft64_tw;
    return pl->blue ? fft64_blue_tables(c, pl) : DS_OK;
}

// One call's device state and its steps; every step works on the planar array x (column stride pl.ld).
struct Fft64Run {
    ds_ctx* c;
    Fft64Plan pl;
    int n_ch;
    double2 *x = nullptr, *tmp = nullptr;
    double *pa = nullptr, *pb = nullptr;  // (n_phase, C) real arrays of the group delay
    dim3 flat(int64_t count) const { return dim3((unsigned)((count + fft64::NT - 1) / fft64::NT)); }
    static size_t phase_bytes(int64_t n_phase, int n_ch) { return 2 * (((size_t)n_phase * n_ch * 8 + 255) & ~size_t(255)); }
    int carve_ws(int64_t n_phase) {
        return carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
            x = cv.take<double2>((size_t)pl.ld * n_ch);
            tmp = cv.take<double2>((size_t)pl.ld * n_ch);
            pa = cv.take<double>((size_t)n_phase * n_ch);
            pb = cv.take<double>((size_t)n_phase * n_ch);
        });
    }
    // the n_cols columns from col0 on (default: all of them) from an (n_in, n_cols) host-order array
    int load(const void* in_dev, bool cplx, int64_t n_in, int col0 = 0, int n_cols = -1) {
        if (n_cols < 0) n_cols = n_ch - col0;
        return launch(c, "fft64_load", fft64::k_load, flat(pl.ld * n_cols), fft64::NT, 0,
                      fft64::LoadArgs{(const double*)in_dev, cplx ? 1 : 0, n_in, pl.n, pl.ld, n_cols, x + (int64_t)col0 * pl.ld});
    }
    int fft(bool inv) {
        using namespace fft64;
        if (!pl.blue) return fft64_pow2(c, pl.tw, x, tmp, pl.n, pl.lg, n_ch, pl.ld, inv);
        auto blue = [&](int mode, const double2* tab, double scale) {
            const int64_t rows = mode == BLUE_POST ? pl.n : pl.ld;
            return launch(c, "fft64_blue", k_blue, flat(rows * n_ch), NT, 0, BlueArgs{x, tab, pl.n, pl.ld, n_ch, mode, inv ? 1 : 0, scale});
        };
        CHK(blue(BLUE_PRE, pl.w, 1.0));
        CHK(fft64_pow2(c, pl.tw, x, tmp, pl.ld, pl.lg, n_ch, pl.ld, false));
        CHK(blue(BLUE_MUL, pl.B, 1.0 / (double)pl.ld));
        CHK(fft64_pow2(c, pl.tw, x, tmp, pl.ld, pl.lg, n_ch, pl.ld, true));
        return blue(BLUE_POST, pl.w, 1.0);
    }
    int point(int mode, double scale) {
        return launch(c, "fft64_point", fft64::k_point, flat(pl.n * n_ch), fft64::NT, 0, fft64::PointArgs{x, pl.n, pl.ld, n_ch, mode, scale});
    }
    int store(int mode, int64_t rows, double scale, void* out_dev) {
        return launch(c, "fft64_store", fft64::k_store, flat(rows * n_ch), fft64::NT, 0,
                      fft64::StoreArgs{x, pl.ld, rows, n_ch, mode, scale, (double*)out_dev});
    }
    // -gradient(unwrap(angle(x[0 .. nb)))) / (2 pi delta_f); with lat_dev [n_ch] (samples) the phase is first
    // wrap(angle + 2 pi f lat / fs), f = k delta_f
    int group_delay(int64_t nb, double delta_f, void* out_dev, const double* lat_dev = nullptr, double fs = 0.0) {
        CHK(store(fft64::STORE_ANGLE, nb, 1.0, pa));
        if (lat_dev)
            CHK(launch(c, "lat_phase", dslat::k_lat_phase, flat(nb * n_ch), dslat::NT, 0,
                       dslat::LatPhaseArgs{pa, nb, n_ch, delta_f, fs, lat_dev}));
        CHK(launch(c, "fft64_unwrap", dssmooth::k_unwrap, dim3((unsigned)n_ch), dssmooth::NT, 0,
                   dssmooth::UnwrapArgs{pa, nb, (int64_t)n_ch, pb}));
        return launch(c, "fft64_gradient", fft64::k_gradient, flat(nb * n_ch), fft64::NT, 0,
                      fft64::GradArgs{pb, nb, n_ch, delta_f, (double*)out_dev});
    }
};

extern "C" int ds_fft_c128(ds_ctx* c, const double* in, int in_complex, int64_t n_in, int n_ch, int64_t n_fft, int inverse,
                           double* out) {
    if (!c || !in || !out) return fail(c, DS_ERR_ARG, "ds_fft_c128: null argument");
    if (n_in < 1) return fail(c, DS_ERR_ARG, "ds_fft_c128: bad shape");
    const size_t e_in = in_complex ? 16 : 8;
    Fft64Run r{c, {}, n_ch};
    // rows of the input past n_fft are never read: they are not uploaded either
    const int64_t n_up = std::min(n_in, std::max<int64_t>(n_fft, 1));
    CHK(fft64_plan(c, "ds_fft_c128", n_fft, n_ch, 0, ((size_t)n_up * e_in + (size_t)n_fft * 16) * (size_t)n_ch, &r.pl));
    CHK(r.carve_ws(0));
    return staged(c, {{e_in, (size_t)n_up * n_ch, in, nullptr}, {16, (size_t)n_fft * n_ch, nullptr, out}}, [&](void* const* d) {
        CHK(r.load(d[0], in_complex != 0, n_up));
        CHK(r.fft(inverse != 0));
        return r.store(fft64::STORE_COMPLEX, n_fft, inverse ? 1.0 / (double)n_fft : 1.0, d[1]);
    });
}

extern "C" int ds_hilbert(ds_ctx* c, const double* x, int64_t n, int n_ch, double* out) {
    if (!c || !x || !out) return fail(c, DS_ERR_ARG, "ds_hilbert: null argument");
    Fft64Run r{c, {}, n_ch};
    CHK(fft64_plan(c, "ds_hilbert", n, n_ch, 0, (size_t)n * 24 * (size_t)n_ch, &r.pl));
    CHK(r.carve_ws(0));
    return staged(c, {{8, (size_t)n * n_ch, x, nullptr}, {16, (size_t)n * n_ch, nullptr, out}}, [&](void* const* d) {
        CHK(r.load(d[0], false, n));
        CHK(r.fft(false));
        CHK(r.point(fft64::POINT_MASK, 1.0));
        CHK(r.fft(true));
        return r.store(fft64::STORE_COMPLEX, n, 1.0 / (double)n, d[1]);
    });
}

extern "C" int ds_cepstrum(ds_ctx* c, const double* x, int64_t n, int n_ch, int complex_cepstrum, double* out) {
    if (!c || !x || !out) return fail(c, DS_ERR_ARG, "ds_cepstrum: null argument");
    Fft64Run r{c, {}, n_ch};
    CHK(fft64_plan(c, "ds_cepstrum", n, n_ch, 0, (size_t)n * 24 * (size_t)n_ch, &r.pl));
    CHK(r.carve_ws(0));
    return staged(c, {{8, (size_t)n * n_ch, x, nullptr}, {16, (size_t)n * n_ch, nullptr, out}}, [&](void* const* d) {
        CHK(r.load(d[0], false, n));
        CHK(r.fft(false));
        CHK(r.point(complex_cepstrum ? fft64::POINT_LOG : fft64::POINT_LOGABS, 1.0));
        CHK(r.fft(true));
        return r.store(fft64::STORE_COMPLEX, n, 1.0 / (double)n, d[1]);
    });
}

extern "C" int ds_from_cepstrum(ds_ctx* c, const double* cepstrum, int64_t n, int n_ch, double* out) {
    if (!c || !cepstrum || !out) return fail(c, DS_ERR_ARG, "ds_from_cepstrum: null argument");
    Fft64Run r{c, {}, n_ch};
    CHK(fft64_plan(c, "ds_from_cepstrum", n, n_ch, 0, (size_t)n * 24 * (size_t)n_ch, &r.pl));
    CHK(r.carve_ws(0));
    return staged(c, {{16, (size_t)n * n_ch, cepstrum, nullptr}, {8, (size_t)n * n_ch, nullptr, out}}, [&](void* const* d) {
        CHK(r.load(d[0], true, n));
        CHK(r.fft(false));
        CHK(r.point(fft64::POINT_EXP, 1.0));
        CHK(r.fft(true));
        return r.store(fft64::STORE_REAL, n, 1.0 / (double)n, d[1]);
    });
}

extern "C" int ds_min_phase(ds_ctx* c, const double* x, int64_t n, int n_ch, int64_t n_fft, int output, int64_t n_out,
                            double delta_f, double* out) {
    if (!c || !x || !out) return fail(c, DS_ERR_ARG, "ds_min_phase: null argument");
    if (n < 1 || output < DS_MIN_PHASE_SPECTRUM || output > DS_MIN_PHASE_GROUP_DELAY)
        return fail(c, DS_ERR_ARG, "ds_min_phase: bad shape or unknown output");
    const int64_t nb = n_fft / 2 + 1;
    const bool gd = output == DS_MIN_PHASE_GROUP_DELAY;
    if (output == DS_MIN_PHASE_IR && (n_out < 1 || n_out > n_fft)) return fail(c, DS_ERR_ARG, "ds_min_phase: n_out outside [1, n_fft]");
    if (gd && (nb < 2 || !(delta_f > 0.0))) return fail(c, DS_ERR_ARG, "ds_min_phase: the group delay needs two bins and delta_f > 0");
    const size_t e_out = output == DS_MIN_PHASE_SPECTRUM ? 16 : 8;
    const int64_t rows = output == DS_MIN_PHASE_SPECTRUM ? n_fft : (output == DS_MIN_PHASE_IR ? n_out : nb);
    Fft64Run r{c, {}, n_ch};
    const int64_t n_up = std::min(n, std::max<int64_t>(n_fft, 1));
    CHK(fft64_plan(c, "ds_min_phase", n_fft, n_ch, gd ? Fft64Run::phase_bytes(nb, n_ch) : 0,
                   ((size_t)n_up * 8 + (size_t)std::max<int64_t>(rows, 0) * e_out) * (size_t)n_ch, &r.pl));
    CHK(r.carve_ws(gd ? nb : 0));
    return staged(c, {{8, (size_t)n_up * n_ch, x, nullptr}, {e_out, (size_t)rows * n_ch, nullptr, out}}, [&](void* const* d) {
        using namespace fft64;
        const double inv_n = 1.0 / (double)n_fft;
        CHK(r.load(d[0], false, n_up));
        CHK(r.fft(false));
        CHK(r.point(POINT_LOGABS, 1.0));
        CHK(r.fft(true));
        CHK(r.point(POINT_FOLD, inv_n));  // the real cepstrum, folded
        CHK(r.fft(false));
        CHK(r.point(POINT_EXP, 1.0));     // the minimum-phase spectrum
        switch (output) {
        case DS_MIN_PHASE_SPECTRUM: return r.store(STORE_COMPLEX, n_fft, 1.0, d[1]);
        case DS_MIN_PHASE_PHASE: return r.store(STORE_ANGLE, nb, 1.0, d[1]);
        case DS_MIN_PHASE_IR:
            CHK(r.fft(true));
            return r.store(STORE_REAL, n_out, inv_n, d[1]);
        default: return r.group_delay(nb, delta_f, d[1]);
        }
    });
}

extern "C" int ds_group_delay_phase(ds_ctx* c, const double* x, int64_t n, int n_ch, double delta_f, double* out) {
    if (!c || !x || !out) return fail(c, DS_ERR_ARG, "ds_group_delay_phase: null argument");
    const int64_t nb = n / 2 + 1;
    if (n < 2 || !(delta_f > 0.0)) return fail(c, DS_ERR_ARG, "ds_group_delay_phase: needs two bins and delta_f > 0");
    Fft64Run r{c, {}, n_ch};
    CHK(fft64_plan(c, "ds_group_delay_phase", n, n_ch, Fft64Run::phase_bytes(nb, n_ch), ((size_t)n + (size_t)nb) * 8 * (size_t)n_ch, &r.pl));
    CHK(r.carve_ws(nb));
    return staged(c, {{8, (size_t)n * n_ch, x, nullptr}, {8, (size_t)nb * n_ch, nullptr, out}}, [&](void* const* d) {
        CHK(r.load(d[0], false, n));
        CHK(r.fft(false));
        return r.group_delay(nb, delta_f, d[1]);
    });
}

extern "C" int ds_group_delay_phase_lat(ds_ctx* c, const double* x, int64_t n, int n_ch, double delta_f,
                                        const double* latency_samples, double fs, double* out) {
    if (!c || !x || !out || !latency_samples) return fail(c, DS_ERR_ARG, "ds_group_delay_phase_lat: null argument");
    const int64_t nb = n / 2 + 1;
    if (n < 2 || !(delta_f > 0.0) || !(fs > 0.0))
        return fail(c, DS_ERR_ARG, "ds_group_delay_phase_lat: needs two bins, delta_f > 0 and fs > 0");
    Fft64Run r{c, {}, n_ch};
    CHK(fft64_plan(c, "ds_group_delay_phase_lat", n, n_ch, Fft64Run::phase_bytes(nb, n_ch),
                   ((size_t)n + (size_t)nb + 1) * 8 * (size_t)n_ch, &r.pl));
    CHK(r.carve_ws(nb));
    return staged(c, {{8, (size_t)n * n_ch, x, nullptr}, {8, (size_t)nb * n_ch, nullptr, out}, {8, (size_t)n_ch, latency_samples}},
                  [&](void* const* d) {
        CHK(r.load(d[0], false, n));
        CHK(r.fft(false));
        return r.group_delay(nb, delta_f, d[1], (const double*)d[2], fs);
    });
}

// ---- latency by cross-correlation (kernels_latency.hpp on the transform above) ---------------------------------------
// Pearson's r per row of the host table rows [n_rows][3] (col_t, col_o, lag), t and o sample-major on the device;
// out_dev [n_rows].  The caller has checked the columns.
static int lag_pearson_run(ds_ctx* c, const char* who, const double* t_dev, int64_t n_t, int n_ch_t, const double* o_dev,
                           int64_t n_o, int n_ch_o, const int64_t* rows, int n_rows, double* out_dev) {
    using namespace dslat;
    const int64_t n_wg = std::max<int64_t>(1, (std::min(n_t, n_o) + dsdist::SPAN - 1) / dsdist::SPAN);  // no span is longer
    if (n_wg > 65535) return fail(c, DS_ERR_UNSUP, who, "signals above 65535 x 4096 samples are not built");
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes,
              {{8, (size_t)n_rows * 3, rows}, {8, (size_t)n_rows * 2}, {8, (size_t)n_rows * n_wg * dsdist::NS}}, t));
    LagArgs a{t_dev, o_dev, n_t, n_o, n_ch_t, n_ch_o, (const int64_t*)t[0], (int)n_wg, nullptr, (double*)t[2], (double*)t[1]};
    const dim3 grid((unsigned)n_rows, (unsigned)n_wg), one((unsigned)n_rows);
    CHK(launch(c, "lag_partial", k_lag_partial<false>, grid, NT, 0, a));
    CHK(launch(c, "lag_final", k_lag_final<false>, one, NT, 0, a));
    a.mean = (const double*)t[1];
    a.out = out_dev;
    CHK(launch(c, "lag_partial@moments", k_lag_partial<true>, grid, NT, 0, a));
    return launch(c, "lag_final@moments", k_lag_final<true>, one, NT, 0, a);
}

extern "C" int ds_lag_pearson(ds_ctx* c, const double* t, int64_t n_t, int n_ch_t, const double* o, int64_t n_o, int n_ch_o,
                              const int64_t* rows, int n_rows, double* out) {
    if (!c || !t || !o || !rows || !out) return fail(c, DS_ERR_ARG, "ds_lag_pearson: null argument");
    if (n_t < 1 || n_o < 1 || n_ch_t < 1 || n_ch_o < 1 || n_rows < 1) return fail(c, DS_ERR_ARG, "ds_lag_pearson: bad shape");
    for (int j = 0; j < n_rows; ++j)
        if (rows[3 * j] < 0 || rows[3 * j] >= n_ch_t || rows[3 * j + 1] < 0 || rows[3 * j + 1] >= n_ch_o)
            return fail(c, DS_ERR_ARG, "ds_lag_pearson: a row names a column that is not there");
    HIPCHK(c, hipSetDevice(c->device));
    return staged(c, {{8, (size_t)n_t * n_ch_t, t}, {8, (size_t)n_o * n_ch_o, o}, {8, (size_t)n_rows, nullptr, out}},
                  [&](void* const* d) {
        return lag_pearson_run(c, "ds_lag_pearson", (const double*)d[0], n_t, n_ch_t, (const double*)d[1], n_o, n_ch_o, rows,
                               n_rows, (double*)d[2]);
    });
}

static int64_t pow2_at_least(int64_t n) {
    int64_t m = 1;
    while (m < n) m <<= 1;
    return m;
}

extern "C" int ds_latency(ds_ctx* c, const double* a, int64_t n_a, int n_ch, const double* b, int64_t n_b, int n_ch_b,
                          int polynomial_points, int reverse_pairs, int64_t* peaks, int64_t* window, double* near,
                          double* pearson) {
    using namespace dslat;
    const char* who = "ds_latency";
    const int p = polynomial_points;
    if (!c || !a || !peaks || (p > 0 && (!window || !near)) || (!b && pearson)) return fail(c, DS_ERR_ARG, who, "null argument");
    if (n_a < 1 || n_ch < 1 || p < 0 || (b && (n_b < 1 || (n_ch_b != n_ch && n_ch_b != 1))))
        return fail(c, DS_ERR_ARG, who, "needs samples, channels (b: as many as a, or one) and polynomial_points >= 0");
    const bool corr = b != nullptr;
    const int cb = corr ? n_ch_b : 0;
    const int64_t L = corr ? n_a + n_b - 1 : n_a, n_fft = pow2_at_least(L);
    if (latency_shape_unsupported(L, (int64_t)n_ch + cb, p))
        return fail(c, DS_ERR_UNSUP, who, "correlations above 2^22 rows, more than 65535 channels in one call or more than 16 "
                                          "polynomial points are not built");
    HIPCHK(c, hipSetDevice(c->device));
    // the device memory of the whole call, for the widest window there can be (all L rows), before anything goes up
    const int n_cand = p > 0 ? 3 : 1, w = 2 * p + 2;
    const int n_wgp = (int)((L + PEAK_SPAN - 1) / PEAK_SPAN);
    const size_t n_win = p > 0 && corr ? (size_t)L * n_ch : 0;
    const size_t io = 8 * ((size_t)n_a * n_ch + (size_t)n_b * cb + n_win + (size_t)n_ch * (1 + w + n_cand));
    const int64_t m2_worst = std::min(pow2_at_least(2 * L - 1), kFft64MaxPow2);
    // the three steps use the workspace one after the other: correlation and peak pairs; the window's two planar arrays
    // (its chirp tables are allocations of their own); Pearson's table, means and block partials
    const size_t ws_corr = (corr ? 2 * (size_t)n_fft * (n_ch + cb) * 16 : 0) + Fft64Run::phase_bytes(n_wgp, n_ch + cb);
    const size_t ws_win = p > 0 ? 2 * (size_t)m2_worst * n_ch * 16 : 0;
    const size_t ws_pearson = pearson ? 8 * (size_t)n_ch * n_cand * (5 + (size_t)(L / dsdist::SPAN + 1) * dsdist::NS) : 0;
    CHK(mem_check(c, who, std::max({ws_corr, ws_win, ws_pearson}), io, p > 0 ? (size_t)(L + 2 * m2_worst) * 16 : 0));
    Fft64Run r1{c, {}, n_ch + cb};
    if (corr) CHK(fft64_plan(c, who, n_fft, n_ch + cb, Fft64Run::phase_bytes(n_wgp, n_ch + cb), io, &r1.pl));
    return staged(c, {{8, (size_t)n_a * n_ch, a}, {8, (size_t)n_b * cb, b}, {8, n_win}, {8, (size_t)n_ch, nullptr, peaks},
                      {8, p > 0 ? (size_t)n_ch * w : 0, nullptr, near}, {8, pearson ? (size_t)n_ch * n_cand : 0, nullptr, pearson}},
                  [&](void* const* d) {
        const double *da = (const double*)d[0], *db = (const double*)d[1];
        int64_t* dpk = (int64_t*)d[3];
        PeakArgs pk{{}, 0, L, n_wgp, nullptr, nullptr, dpk};
        if (corr) {
            // both signals as columns of one batch; the workgroups' peak pairs take the place of the run's phase arrays
            CHK(r1.carve_ws(n_wgp));
            CHK(r1.load(da, false, n_a, 0, n_ch));
            CHK(r1.load(db, false, n_b, n_ch, cb));
            CHK(r1.fft(false));
            CHK(launch(c, "lat_xmul", k_xmul, r1.flat(n_fft * n_ch), NT, 0, XmulArgs{r1.x, n_fft, r1.pl.ld, n_ch, cb}));
            r1.n_ch = n_ch;  // the products lie in the leading columns
            CHK(r1.fft(true));
            pk.in = RowView{(const double*)r1.x, 2 * r1.pl.ld, 2, n_fft - (n_a - 1), n_fft};
            pk.pv = r1.pa;
            pk.pi = (int64_t*)r1.pb;
        } else {
            void* t[kMaxStaged];
            CHK(stage(c, &c->ws, &c->ws_bytes, {{8, (size_t)n_ch * n_wgp}, {8, (size_t)n_ch * n_wgp}}, t));
            pk.in = RowView{da, 1, n_ch, 0, n_a};
            pk.pv = (double*)t[0];
            pk.pi = (int64_t*)t[1];
        }
        CHK(launch(c, "lat_peak", k_peak, dim3((unsigned)n_wgp, (unsigned)n_ch), NT, 0, pk));
        CHK(launch(c, "lat_peak_final", k_peak_final, dim3((unsigned)n_ch), NT, 0, pk));
        // the window's bounds depend on the peaks: the one read-back in the middle of the call
        std::vector<int64_t> hp((size_t)n_ch);
        CHK(ds_download(c, hp.data(), dpk, (size_t)n_ch * 8));
        if (p > 0) {
            const int64_t d_min = *std::min_element(hp.begin(), hp.end()), d_max = *std::max_element(hp.begin(), hp.end());
            const int64_t lo = std::max<int64_t>(d_min - 200, 0), m = std::min(d_max + 200, L) - lo;
            window[0] = lo;
            window[1] = m;
            if (fft64_len_unsupported(m))
                return fail(c, DS_ERR_UNSUP, who, "the window around the peaks is longer than 2^21 rows and no power of two: "
                                                  "transform lengths above 2^22 (powers of two) or 2^21 (any other) are not built");
            const double* src = da + lo * n_ch;
            if (corr) {
                CHK(launch(c, "lat_window", k_window, r1.flat(m * n_ch), NT, 0,
                           WindowArgs{pk.in, lo, m, n_ch, 1.0 / (double)n_fft, (double*)d[2]}));
                src = (const double*)d[2];
            }
            // the window is out of the workspace: the second run may lay its tables and arrays over the first one's
            Fft64Run r2{c, {}, n_ch};
            CHK(fft64_plan(c, who, m, n_ch, 0, io, &r2.pl));
            CHK(r2.carve_ws(0));
            CHK(r2.load(src, false, m));
            CHK(r2.fft(false));
            CHK(r2.point(fft64::POINT_MASK, 1.0));
            CHK(r2.fft(true));
            CHK(launch(c, "lat_near", k_near, r2.flat((int64_t)n_ch * w), NT, 0,
                       NearArgs{r2.x, r2.pl.ld, m, lo, dpk, n_ch, p, (double*)d[4]}));
        }
        if (!pearson) return DS_OK;
        // entry j pairs column j of b (or its only one) with column j of a, at the lags around the peak of column j -- or,
        // reverse_pairs, of column n_ch - 1 - j
        std::vector<int64_t> rows((size_t)n_ch * n_cand * 3);
        for (int j = 0; j < n_ch; ++j)
            for (int k = 0; k < n_cand; ++k) {
                int64_t* row = &rows[((size_t)j * n_cand + k) * 3];
                row[0] = cb == 1 ? 0 : j;
                row[1] = j;
                row[2] = n_a - 1 - hp[reverse_pairs ? n_ch - 1 - j : j] + (n_cand == 3 ? k - 1 : 0);
            }
        return lag_pearson_run(c, who, db, n_b, cb, da, n_a, n_ch, rows.data(), n_ch * n_cand, (double*)d[5]);
    });
}

// ---- frequency-weighted segmental SNR (kernels_dist.hpp on kernels_ciir.hpp and the transform above) ---------------
// Everything ds_fw_snr_seg and ds_fw_snr_seg_dev share.
struct FwCall {
    const char* who;
    int n_ch_x, n_ch;
    int64_t n;
    const double* sos;     // host [n_band][n_sec][6] complex128: the gammatone bank
    int n_band, n_sec;
    const double* window;  // host [lw]
    int lw;
    double lo, hi, gamma;
    int chunk_frames;
    int64_t hop() const { return lw / 2; }
    int64_t n_frames() const { return (n + hop() - 1) / hop(); }
    int64_t cols_per_frame() const { return (int64_t)n_band * n_ch; }
    int64_t chunk() const {
        return std::max<int64_t>(1, std::min<int64_t>({chunk_frames > 0 ? chunk_frames : 32, 65535 / cols_per_frame(), n_frames()}));
    }
};

static int fw_check(ds_ctx* c, const FwCall& q, const void* x, const void* xhat, const void* out) {
    if (!c || !x || !xhat || !out || !q.sos || !q.window) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n < 1 || q.n_ch < 1 || (q.n_ch_x != q.n_ch && q.n_ch_x != 1) || q.n_band < 1 || q.n_sec < 1 || q.lw < 2 || q.lw % 2 ||
        !(q.lo <= q.hi) || !std::isfinite(q.gamma) || q.chunk_frames < 0)
        return fail(c, DS_ERR_ARG, q.who, "needs samples, channels (x: as many as xhat, or one), bands, an even window, "
                                          "an ordered range and a finite gamma");
    if (q.lw > 16384) return fail(c, DS_ERR_UNSUP, q.who, "windows above 16384 samples are not built (the bins' sums are held in LDS)");
    if (q.cols_per_frame() > 65535) return fail(c, DS_ERR_UNSUP, q.who, "more than 65535 (band, channel) pairs is not built");
    const CiirCall f{q.who, q.n_ch, q.n, q.sos, q.n_band, q.n_sec};
    return ciir_check(c, f, x, out);
}

// x, xhat: device samples of either type, sample n of channel ch at x[ch sc + n ss]; out_dev [n_ch]
template <typename T>
static int fw_run(ds_ctx* c, const FwCall& q, Fft64Run& r, const CiirTables& tb, const T* x, int64_t sxc, int64_t sxn,
                  const T* xhat, int64_t shc, int64_t shn, double* out_dev) {
    using namespace dsdist;
    const CiirCall fx{q.who, q.n_ch_x, q.n, q.sos, q.n_band, q.n_sec}, fh{q.who, q.n_ch, q.n, q.sos, q.n_band, q.n_sec};
    const int64_t chunk = q.chunk(), n_frames = q.n_frames();
    CiirDev dv;
    double *xb, *xhb, *win, *frames;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        ciir_take(cv, fh, &dv);  // (xhat has no fewer channels than x: its group states hold either run)
        xb = cv.take<double>((size_t)q.n_band * q.n_ch_x * q.n);
        xhb = cv.take<double>((size_t)q.n_band * q.n_ch * q.n);
        win = cv.take<double>((size_t)q.lw);
        frames = cv.take<double>((size_t)n_frames * q.n_ch);
        r.x = cv.take<double2>((size_t)r.pl.ld * chunk * q.cols_per_frame());
        r.tmp = cv.take<double2>((size_t)r.pl.ld * chunk * q.cols_per_frame());
    }));
    CHK(ciir_upload(c, tb, dv));
    CHK(ds_upload(c, win, q.window, (size_t)q.lw * 8));
    // the real parts of the bank's outputs, float64 planar (band, channel, sample)
    CHK(ciir_run<T>(c, fx, dv, x, sxc, sxn, nullptr, xb, nullptr, (int64_t)q.n_ch_x * q.n, q.n, 1, nullptr));
    CHK(ciir_run<T>(c, fh, dv, xhat, shc, shn, nullptr, xhb, nullptr, (int64_t)q.n_ch * q.n, q.n, 1, nullptr));
    for (int64_t m0 = 0; m0 < n_frames; m0 += chunk) {
        const int64_t nf = std::min(chunk, n_frames - m0), cols = nf * q.cols_per_frame();
        r.n_ch = (int)cols;
        CHK(launch(c, "fw_frame", k_fw_frame, dim3((unsigned)((q.lw + NT - 1) / NT), (unsigned)cols), NT, 0,
                   FrameArgs{xb, xhb, win, q.n, q.hop(), m0, q.lw, q.n_band, q.n_ch, q.n_ch_x, cols, r.pl.ld, r.x}));
        CHK(r.fft(false));
        CHK(launch(c, "fw_reduce", k_fw_reduce, dim3((unsigned)nf, (unsigned)q.n_ch), NT, fw_reduce_lds_bytes(q.lw),
                   ReduceArgs{r.x, r.pl.ld, q.lw, q.n_band, q.n_ch, q.gamma, q.lo, q.hi, m0, frames}));
    }
    hipLaunchKernelGGL(k_fw_mean, dim3((unsigned)q.n_ch), dim3(NT), 0, c->stream, (const double*)frames, n_frames, q.n_ch, out_dev);
    HIPCHK(c, hipGetLastError());
    return DS_OK;
}

// the checks, the memory pre-check (inside fft64_plan) and the host tables: nothing is uploaded before they pass
static int fw_plan(ds_ctx* c, const FwCall& q, size_t io, Fft64Run* r, CiirTables* tb) {
    if (!ciir_tables(q.sos, q.n_band, q.n_sec, tb->coef, tb->phi, tb->phig))
        return fail(c, DS_ERR_ARG, q.who, "sections must be finite with a0 != 0");
    HIPCHK(c, hipSetDevice(c->device));
    Carver probe;
    CiirDev dv;
    ciir_take(probe, CiirCall{q.who, q.n_ch, q.n, q.sos, q.n_band, q.n_sec}, &dv);
    const size_t extra = probe.off + 8 * ((size_t)q.n_band * (q.n_ch_x + q.n_ch) * q.n + q.lw + (size_t)q.n_frames() * q.n_ch) + 8 * 256;
    r->c = c;
    r->n_ch = (int)(q.chunk() * q.cols_per_frame());
    return fft64_plan(c, q.who, q.lw, r->n_ch, extra, io, &r->pl);
}

// host pointers: x (n, n_ch_x), xhat (n, n_ch) float64; out (n_ch)
extern "C" int ds_fw_snr_seg(ds_ctx* c, const double* x, int n_ch_x, const double* xhat, int n_ch, int64_t n, const double* sos,
                             int n_band, int n_sec, const double* window, int window_length, double snr_lo_db, double snr_hi_db,
                             double gamma, int chunk_frames, double* out) {
    const FwCall q{"ds_fw_snr_seg", n_ch_x, n_ch, n, sos, n_band, n_sec, window, window_length, snr_lo_db, snr_hi_db, gamma, chunk_frames};
    CHK(fw_check(c, q, x, xhat, out));
    Fft64Run r{c, {}, 0};
    CiirTables tb;
    CHK(fw_plan(c, q, 8 * ((size_t)n * (n_ch_x + n_ch) + n_ch), &r, &tb));
    return staged(c, {{8, (size_t)n * n_ch_x, x}, {8, (size_t)n * n_ch, xhat}, {8, (size_t)n_ch, nullptr, out}}, [&](void* const* d) {
        return fw_run<double>(c, q, r, tb, (const double*)d[0], 1, n_ch_x, (const double*)d[1], 1, n_ch, (double*)d[2]);
    });
}

// device-resident planar float32 signals, channel ch at x_dev + ch ldx
extern "C" int ds_fw_snr_seg_dev(ds_ctx* c, const float* x, int n_ch_x, int64_t ldx, const float* xhat, int n_ch, int64_t ldxh,
                                 int64_t n, const double* sos, int n_band, int n_sec, const double* window, int window_length,
                                 double snr_lo_db, double snr_hi_db, double gamma, int chunk_frames, double* out) {
    const FwCall q{"ds_fw_snr_seg_dev", n_ch_x, n_ch, n, sos, n_band, n_sec, window, window_length, snr_lo_db, snr_hi_db, gamma, chunk_frames};
    CHK(fw_check(c, q, x, xhat, out));
    if (ldx < n || ldxh < n) return fail(c, DS_ERR_ARG, q.who, "row stride below the sample count");
    Fft64Run r{c, {}, 0};
    CiirTables tb;
    CHK(fw_plan(c, q, 8 * (size_t)n_ch, &r, &tb));
    return staged(c, {{8, (size_t)n_ch, nullptr, out}}, [&](void* const* d) {
        return fw_run<float>(c, q, r, tb, x, ldx, 1, xhat, ldxh, 1, (double*)d[0]);
    });
}

// ---- linear prediction (kernels_lpc.hpp), float64 ------------------------------------------------------------
// Everything ds_lpc and ds_lpc_dev share.
struct LpcCall {
    const char* who;
    int64_t n_samples;
    int n_ch;
    const double* window;  // host [L]
    int L;
    int64_t hop;
    int order, method;
    double *a, *var;       // host (order + 1, n_frames, n_ch), (n_frames, n_ch)
    int* singular;         // host
    int64_t n_frames;      // ceil(n_samples / hop): set by lpc_check
    size_t pairs() const { return (size_t)n_frames * (size_t)n_ch; }
};

// shape, bounds and work guard, then the pointers; nothing touches the device
static int lpc_check(ds_ctx* c, LpcCall& q, const void* x) {
    if (q.n_samples < 1 || q.n_ch < 1 || q.L < 2 || q.hop < 1 || q.order < 1 || q.order >= q.L)
        return fail(c, DS_ERR_ARG, q.who, "needs samples, channels, hop >= 1 and 1 <= order < window length");
    if (q.method != DS_LPC_YULE_WALKER && q.method != DS_LPC_BURG) return fail(c, DS_ERR_ARG, q.who, "unknown method");
    q.n_frames = q.n_samples / q.hop + (q.n_samples % q.hop != 0);
    if (q.n_frames > kLpcMaxPairs / q.n_ch || lpc_shape_unsupported(q.L, q.order, q.n_frames * q.n_ch))
        return fail(c, DS_ERR_UNSUP, q.who, "windows above 8192 samples, orders above 255 or 2^31 (frame, channel) pairs are not built");
    if (lpc_work_too_large(q.n_frames * q.n_ch, q.L, q.order))
        return fail(c, DS_ERR_UNSUP, q.who, "frames x channels x window x (order + 1) is beyond the work bound");
    if (!c || !x || !q.window || !q.a || !q.var || !q.singular) return fail(c, DS_ERR_ARG, q.who, "null argument");
    return DS_OK;
}

template <typename T>
static int lpc_launch(ds_ctx* c, const LpcCall& q, const T* x, int64_t ss, int64_t cs, const double* dw, double* da,
                      double* dvar, int* dflag) {
    using namespace dslpc;
    CHK(ds_memset(c, dflag, 0, 4));
    const LpcArgs a{x, ss, cs, q.n_samples, q.n_ch, q.n_frames, dw, q.L, q.hop, q.order, da, dvar, dflag};
    const dim3 grid((unsigned)q.pairs());
    if (q.method == DS_LPC_BURG) return launch(c, "lpc_burg", k_lpc_burg<T>, grid, NT, burg_lds_bytes(q.L), a);
    return launch(c, "lpc_yw", k_lpc_yw<T>, grid, NT, yw_lds_bytes(q.L), a);
}

extern "C" int ds_lpc(ds_ctx* c, const double* x, int64_t n_samples, int n_ch, const double* window, int window_length,
                      int64_t hop, int order, int method, double* a, double* var, int* singular) {
    LpcCall q{"ds_lpc", n_samples, n_ch, window, window_length, hop, order, method, a, var, singular, 0};
    CHK(lpc_check(c, q, x));
    const size_t nx = (size_t)n_samples * n_ch, na = (size_t)(order + 1) * q.pairs();
    CHK(mem_check(c, q.who, 0, (nx + (size_t)q.L + na + q.pairs()) * 8 + 4, 0));
    return staged(c, {{8, nx, x, nullptr}, {8, (size_t)q.L, window, nullptr}, {8, na, nullptr, a}, {8, q.pairs(), nullptr, var},
                      {4, 1, nullptr, singular}}, [&](void* const* d) {
        return lpc_launch<double>(c, q, (const double*)d[0], n_ch, 1, (const double*)d[1], (double*)d[2], (double*)d[3], (int*)d[4]);
    });
}

extern "C" int ds_lpc_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_samples, const double* window,
                          int window_length, int64_t hop, int order, int method, double* a, double* var, int* singular) {
    LpcCall q{"ds_lpc_dev", n_samples, n_ch, window, window_length, hop, order, method, a, var, singular, 0};
    CHK(lpc_check(c, q, x));
    if (ldx < n_samples) return fail(c, DS_ERR_ARG, "ds_lpc_dev: ldx < n_samples");
    const size_t na = (size_t)(order + 1) * q.pairs();
    CHK(mem_check(c, q.who, (size_t)q.L * 8, (na + q.pairs()) * 8 + 4, 0));
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, (size_t)q.L, window}}, t));
    return staged(c, {{8, na, nullptr, a}, {8, q.pairs(), nullptr, var}, {4, 1, nullptr, singular}}, [&](void* const* d) {
        return lpc_launch<float>(c, q, x, 1, ldx, (const double*)t[0], (double*)d[0], (double*)d[1], (int*)d[2]);
    });
}

// r: host (order + 1, n_cols); a: host (order + 1, n_cols) with a[0] = 1; var: host (n_cols)
extern "C" int ds_levinson(ds_ctx* c, const double* r, int order, int64_t n_cols, double* a, double* var, int* singular) {
    if (order < 1 || n_cols < 1) return fail(c, DS_ERR_ARG, "ds_levinson: needs order >= 1 and a column");
    if (order > kLpcMaxOrder || n_cols > kLpcMaxPairs)
        return fail(c, DS_ERR_UNSUP, "ds_levinson: orders above 255 or 2^31 columns are not built");
    if (!c || !r || !a || !var || !singular) return fail(c, DS_ERR_ARG, "ds_levinson: null argument");
    const size_t nr = (size_t)(order + 1) * (size_t)n_cols;
    CHK(mem_check(c, "ds_levinson", 0, (2 * nr + (size_t)n_cols) * 8 + 4, 0));
    return staged(c, {{8, nr, r, nullptr}, {8, nr, nullptr, a}, {8, (size_t)n_cols, nullptr, var}, {4, 1, nullptr, singular}},
                  [&](void* const* d) {
        CHK(ds_memset(c, d[3], 0, 4));
        return launch(c, "lpc_levinson", dslpc::k_levinson, dim3((unsigned)n_cols), 64, 0,
                      dslpc::LevinsonArgs{(const double*)d[0], order, n_cols, (double*)d[1], (double*)d[2], (int*)d[3]});
    });
}

// a: host (order + 1, n_frames, n_ch); sources: host (window_length, n_frames, n_ch); y: host (n_out, n_ch)
extern "C" int ds_lpc_synth(ds_ctx* c, const double* a, const double* sources, const double* window, int window_length,
                            int64_t n_frames, int n_ch, int64_t hop, int order, int64_t n_out, double* y) {
    using namespace dslpc;
    const int L = window_length;
    if (n_frames < 1 || n_ch < 1 || L < 2 || hop < 1 || order < 1 || order >= L || n_out < 1)
        return fail(c, DS_ERR_ARG, "ds_lpc_synth: needs frames, channels, output samples, hop >= 1 and 1 <= order < window length");
    if (n_frames > kLpcMaxPairs / n_ch || lpc_shape_unsupported(L, order, n_frames * n_ch) ||
        n_out > kLpcMaxPairs * (int64_t)NT / n_ch)
        return fail(c, DS_ERR_UNSUP, "ds_lpc_synth: windows above 8192 samples, orders above 255 or 2^31 (frame, channel) pairs are not built");
    if (lpc_work_too_large(n_frames * n_ch, L, order))
        return fail(c, DS_ERR_UNSUP, "ds_lpc_synth: frames x channels x window x (order + 1) is beyond the work bound");
    if (!c || !a || !sources || !window || !y) return fail(c, DS_ERR_ARG, "ds_lpc_synth: null argument");
    const size_t pairs = (size_t)n_frames * n_ch, na = (size_t)(order + 1) * pairs, ns = (size_t)L * pairs;
    const size_t ny = (size_t)n_out * n_ch;
    CHK(mem_check(c, "ds_lpc_synth", ns * 8, (na + ns + (size_t)L + ny) * 8, 0));
    double* yf;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) { yf = cv.take<double>(ns); }));
    return staged(c, {{8, na, a, nullptr}, {8, ns, sources, nullptr}, {8, (size_t)L, window, nullptr}, {8, ny, nullptr, y}},
                  [&](void* const* d) {
        CHK(launch(c, "lpc_filter", k_lpc_filter, dim3((unsigned)((pairs + FILT_WAVES - 1) / FILT_WAVES)), 64 * FILT_WAVES, 0,
                   FilterArgs{(const double*)d[0], (const double*)d[1], L, (int64_t)pairs, order, yf}));
        return launch(c, "lpc_ola", k_lpc_ola, dim3((unsigned)((ny + NT - 1) / NT)), NT, 0,
                      OlaArgs{yf, (const double*)d[2], L, n_frames, n_ch, hop, n_out, (double*)d[3]});
    });
}

// ---- the all-pass table of warp and laguerre (kernels_warp.hpp, warp_plan.hpp), float64 ---------------------------
// Everything ds_allpass_table and ds_allpass_table_dev share.
struct AllpassCall {
    const char* who;
    int64_t n_in;
    int n_ch;
    double p, q;
    const double *row0, *col0;  // host [n_out], [n_in]
    int64_t n_out;
    double* out;                // host (n_out, n_ch)
    int groups() const { return (n_ch + dswarp::G - 1) / dswarp::G; }
};

// shape, bounds and work guard, then the pointers; nothing touches the device
static int allpass_check(ds_ctx* c, const AllpassCall& q, const void* x) {
    if (q.n_in < 1 || q.n_out < 1 || q.n_ch < 1 || !std::isfinite(q.p) || !std::isfinite(q.q))
        return fail(c, DS_ERR_ARG, q.who, "needs input samples, output samples, channels and finite p and q");
    if (warp_shape_unsupported(q.n_in, q.n_out, q.n_ch))
        return fail(c, DS_ERR_UNSUP, q.who, "tables above 131072 samples a side or 65536 channels are not built");
    if (warp_work_too_large(q.n_in, q.n_out, q.groups()))
        return fail(c, DS_ERR_UNSUP, q.who, "input samples x output samples x channel groups is beyond the work bound");
    if (!c || !x || !q.row0 || !q.col0 || !q.out) return fail(c, DS_ERR_ARG, q.who, "null argument");
    return DS_OK;
}

// the boundary image goes to c->ws, then one grid per tile anti-diagonal
template <typename T>
static int allpass_launch(ds_ctx* c, const AllpassCall& q, const T* x, int64_t ss, int64_t cs, double* out) {
    using namespace dswarp;
    const dswarp::Plan pl = make_plan(q.n_in, q.n_out);
    std::vector<double> init((size_t)workspace_doubles(pl));
    initial_image(pl, q.row0, q.col0, init.data());
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, init.size(), init.data()}}, t));
    for (int64_t d = 0; d < pl.launches; ++d) {
        const TileArgs a{x, ss, cs, q.n_ch, q.p, q.q, (double*)t[0], out, pl, d};
        CHK(launch(c, "allpass_tile", k_allpass_tile<T>, dim3((unsigned)diagonal(pl, d).count, (unsigned)q.groups()), TJ,
                   tile_lds_bytes(), a));
    }
    return DS_OK;
}

extern "C" int ds_allpass_table(ds_ctx* c, const double* x, int64_t n_in, int n_ch, double p, double q, const double* row0,
                                const double* col0, int64_t n_out, double* out) {
    AllpassCall k{"ds_allpass_table", n_in, n_ch, p, q, row0, col0, n_out, out};
    CHK(allpass_check(c, k, x));
    const size_t nx = (size_t)n_in * n_ch, no = (size_t)n_out * n_ch;
    CHK(mem_check(c, k.who, (size_t)dswarp::workspace_doubles(dswarp::make_plan(n_in, n_out)) * 8, (nx + no) * 8, 0));
    return staged(c, {{8, nx, x, nullptr}, {8, no, nullptr, out}}, [&](void* const* d) {
        return allpass_launch<double>(c, k, (const double*)d[0], n_ch, 1, (double*)d[1]);
    });
}

extern "C" int ds_allpass_table_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_in, double p, double q,
                                    const double* row0, const double* col0, int64_t n_out, double* out) {
    AllpassCall k{"ds_allpass_table_dev", n_in, n_ch, p, q, row0, col0, n_out, out};
    CHK(allpass_check(c, k, x));
    if (ldx < n_in) return fail(c, DS_ERR_ARG, "ds_allpass_table_dev: ldx < n_in");
    const size_t no = (size_t)n_out * n_ch;
    CHK(mem_check(c, k.who, (size_t)dswarp::workspace_doubles(dswarp::make_plan(n_in, n_out)) * 8, no * 8, 0));
    return staged(c, {{8, no, nullptr, out}}, [&](void* const* d) {
        return allpass_launch<float>(c, k, x, 1, ldx, (double*)d[0]);
    });
}

// ---- structure filters: lattice-ladder, warped and Kautz recursions (kernels_sfilt.hpp) ---------------------------------
// Everything ds_sfilt and ds_sfilt_dev share.  ldx, ld_y: the _dev entry's row strides (the host entry's rows are dense).
struct SfiltCall {
    const char* who;
    int n_ch;
    int64_t n_samples, ldx, ld_y;
    int kind, d, aux;
    const double* coef;  // host, packed as kernels_sfilt.hpp lays it out
    int64_t n_groups() const { return (n_samples + sfilt::G - 1) / sfilt::G; }
    size_t n_coef() const { return (size_t)sfilt::coef_count(kind, d, aux); }
    size_t ws_bytes() const {  // coefficients, Phi, Phi^B, group states: four 256-byte aligned pieces
        return (n_coef() + 2 * (size_t)d * d + (size_t)n_ch * (size_t)n_groups() * d) * 8 + 4 * 256;
    }
};

// shape and bounds; nothing touches the device
static int sfilt_check(ds_ctx* c, const SfiltCall& q, const void* x, const void* y) {
    if (!c || !x || !y || !q.coef) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_ch <= 0 || q.n_samples <= 0 || q.d <= 0 || q.ldx < q.n_samples || q.ld_y < q.n_samples)
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (q.kind < 0 || q.kind >= sfilt::N_KINDS) return fail(c, DS_ERR_ARG, q.who, "unknown structure kind");
    if (q.d > sfilt::MAX_D)
        return fail(c, DS_ERR_UNSUP, q.who, "more than 64 states in one structure is not built (the carry's state "
                                            "vector is one value per lane of a wave)");
    if ((q.kind == sfilt::SOS_LATTICE && q.d % 2) || (q.kind == sfilt::WARPED_IIR && (q.aux < 1 || q.aux > q.d)) ||
        (q.kind == sfilt::KAUTZ && (q.aux < 0 || q.aux > q.d || (q.d - q.aux) % 2)))
        return fail(c, DS_ERR_ARG, q.who, "the state count does not fit the structure");
    CHK(carry_limits(c, q.who, q.n_ch, q.n_samples, "more than 65535 channels is not built yet"));
    for (size_t i = 0; i < q.n_coef(); ++i)
        if (!std::isfinite(q.coef[i])) return fail(c, DS_ERR_ARG, q.who, "coefficients must be finite");
    return DS_OK;
}

// Host side of the carry: column j of the zero-input transition A is one step of the structure's own step function from
// the unit state e_j with x = 0 (exact: a zero-input step is linear); Phi = A^L and Phi^B by squaring.  The carry gain is
// the largest magnitude in the two; above sfilt::max_gain(kind) the carried states' rounding is no longer small beside the
// output, and a recursion that is not stable ends there or at a non-finite power.
struct SfiltTables {
    std::vector<double> phi, phig;
};
static int sfilt_tables(ds_ctx* c, const SfiltCall& q, SfiltTables& tb) {
    const int d = q.d;
    std::vector<double> a((size_t)d * d, 0.0), st((size_t)d);
    for (int j = 0; j < d; ++j) {
        std::fill(st.begin(), st.end(), 0.0);
        st[j] = 1.0;
        (void)sfilt::step(q.kind, 0.0, st.data(), q.coef, d, q.aux);
        for (int i = 0; i < d; ++i) a[(size_t)i * d + j] = st[i];
    }
    carry::carry_powers(a, d, tb.phi, tb.phig);
    double gain = 0.0;
    for (const std::vector<double>* m : {&tb.phi, &tb.phig})
        for (double v : *m) gain = std::isfinite(v) ? std::max(gain, std::fabs(v)) : INFINITY;
    if (!(gain <= sfilt::max_gain(q.kind)))
        return fail(c, DS_ERR_UNSUP, q.who, "the recursion's carry gain (largest magnitude in Phi = A^32 and Phi^64) is "
                                            "above the limit: an unstable or too ill-conditioned structure is not run "
                                            "time-parallel");
    return DS_OK;
}

// the three passes over device buffers of either sample type; y element (c, n) at y[c syc + n syn]; zi, zf: device
// arrays [D][n_ch] or nullptr
template <typename T>
static int sfilt_run(ds_ctx* c, const SfiltCall& q, const SfiltTables& tb, const T* x, int64_t sxc, int64_t sxn,
                     const double* zi, T* y, int64_t syc, int64_t syn, double* zf) {
    const int d = q.d, n_ch = q.n_ch;
    const int64_t n_groups = q.n_groups();
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, q.n_coef(), q.coef}, {8, tb.phi.size(), tb.phi.data()},
                                        {8, tb.phig.size(), tb.phig.data()}, {8, (size_t)n_ch * n_groups * d}}, t));
    const double *dcoef = (const double*)t[0], *dphi = (const double*)t[1], *dphig = (const double*)t[2];
    double* gst = (double*)t[3];
    sfilt::Args<T> a{x, sxc, sxn, y, syc, syn, q.n_samples, n_ch, q.kind, d, q.aux, n_groups, dcoef, dphi, dphig, gst, zi, zf};
    if (n_groups > 1)
        CHK(launch(c, "sfilt_group", sfilt::k_sfilt_group<T>, dim3((unsigned)(n_groups - 1), (unsigned)n_ch), sfilt::B,
                   sfilt::lds_bytes(d, false), a));
    carry::CarryArgs ca{dphig, gst, zi, n_groups, n_ch, d};  // one filter: zi [D][n_ch]
    CHK(launch(c, "sfilt_carry", carry::k_block_carry, dim3((unsigned)n_ch), sfilt::B, sizeof(double) * d * d, ca));
    return launch(c, "sfilt_apply", sfilt::k_sfilt_apply<T>, dim3((unsigned)n_groups, (unsigned)n_ch), sfilt::B,
                  sfilt::lds_bytes(d, true), a);
}

// device-resident planar float32 samples; coef, zi and zf stay host pointers (zi / zf [D][n_ch] cross through c->io)
extern "C" int ds_sfilt_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_samples, int kind,
                            const double* coef, int d, int aux, const double* zi, float* y, int64_t ld_y, double* zf) {
    const SfiltCall q{"ds_sfilt_dev", n_ch, n_samples, ldx, ld_y, kind, d, aux, coef};
    CHK(sfilt_check(c, q, x, y));
    SfiltTables tb;
    CHK(sfilt_tables(c, q, tb));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nz = (size_t)d * n_ch;
    CHK(mem_check(c, q.who, q.ws_bytes(), 2 * nz * 8, 0));
    return staged(c, {{8, nz, zi}, {8, zf ? nz : 0, nullptr, zf}}, [&](void* const* dv) {
        return sfilt_run<float>(c, q, tb, x, ldx, 1, zi ? (const double*)dv[0] : nullptr, y, ld_y, 1,
                                zf ? (double*)dv[1] : nullptr);
    });
}

// host pointers in the reference's layouts: x and y (n_samples, n_ch) float64; the samples cross the link as they are
// and the kernels read them with the channel stride
extern "C" int ds_sfilt(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, int kind, const double* coef, int d,
                        int aux, const double* zi, double* y, double* zf) {
    const SfiltCall q{"ds_sfilt", n_ch, n_samples, n_samples, n_samples, kind, d, aux, coef};
    CHK(sfilt_check(c, q, x, y));
    SfiltTables tb;
    CHK(sfilt_tables(c, q, tb));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nx = (size_t)n_ch * n_samples, nz = (size_t)d * n_ch;
    CHK(mem_check(c, q.who, q.ws_bytes(), (2 * nx + 2 * nz) * 8, 0));
    return staged(c, {{8, nx, x}, {8, nx, nullptr, y}, {8, nz, zi}, {8, zf ? nz : 0, nullptr, zf}}, [&](void* const* dv) {
        return sfilt_run<double>(c, q, tb, (const double*)dv[0], 1, n_ch, zi ? (const double*)dv[2] : nullptr,
                                 (double*)dv[1], 1, n_ch, zf ? (double*)dv[3] : nullptr);
    });
}

// ---- realtime filters: state-variable, transposed direct form II, parallel sections, state space; the direct FIR sum
// (kernels_rtfilt.hpp) ------------------------------------------------------------------------------------------------
// The FIR sum's bounds and its padded taps.  Nothing touches the device.
struct RtFir {
    const char* who;
    const double* b;  // host, n_taps values
    int n_taps;
    int order() const { return n_taps - 1; }
    int nt4() const { return rtfilt::fir_nt4(order()); }
    std::vector<double> padded() const {
        std::vector<double> t((size_t)nt4(), 0.0);
        std::copy(b, b + n_taps, t.begin());
        return t;
    }
};
static int rtfir_check(ds_ctx* c, const RtFir& f, int n_ch, int64_t n_samples) {
    if (!f.b || f.n_taps < 1) return fail(c, DS_ERR_ARG, f.who, "the FIR part needs at least one tap");
    if (f.n_taps > rtfilt::FIR_MAX_TAPS)
        return fail(c, DS_ERR_UNSUP, f.who, "more than 4096 taps is not built in the direct FIR sum");
    if ((double)n_samples * (double)n_ch * (double)f.n_taps > 1099511627776.0)
        return fail(c, DS_ERR_UNSUP, f.who, "more than 2^40 multiply-adds (samples x channels x taps) in one call of the "
                                            "direct FIR sum is not built");
    if (n_ch > 65535) return fail(c, DS_ERR_UNSUP, f.who, "more than 65535 channels is not built yet");
    for (int i = 0; i < f.n_taps; ++i)
        if (!std::isfinite(f.b[i])) return fail(c, DS_ERR_ARG, f.who, "coefficients must be finite");
    return DS_OK;
}

// the launch over device buffers; taps [nt4] and hist [n_ch][order] (or nullptr) are device arrays
template <typename TI, typename TO>
static int rtfir_launch(ds_ctx* c, const RtFir& f, const TI* x, int64_t sxc, int64_t sxn, int64_t n, int n_ch,
                        const double* taps, const double* hist, TO* y, int64_t syc, int64_t syn) {
    const rtfilt::FirArgs<TI, TO> a{x, sxc, sxn, y, syc, syn, n, n_ch, f.order(), f.nt4(), taps, hist};
    return launch(c, "rtfir", rtfilt::k_rtfir<TI, TO>, dim3((unsigned)((n + rtfilt::FIR_TILE - 1) / rtfilt::FIR_TILE), (unsigned)n_ch),
                  rtfilt::FIR_NT, rtfilt::fir_lds_bytes(f.nt4()), a);
}

template <typename T>
static int rtfir_run(ds_ctx* c, const RtFir& f, const T* x, int64_t sxc, int64_t sxn, int64_t n, int n_ch, const double* hist,
                     T* y, int64_t syc, int64_t syn) {
    const std::vector<double> taps = f.padded();
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, taps.size(), taps.data()}, {8, hist ? (size_t)n_ch * f.order() : 0, hist}}, t));
    return rtfir_launch<T, T>(c, f, x, sxc, sxn, n, n_ch, (const double*)t[0], hist && f.order() ? (const double*)t[1] : nullptr,
                              y, syc, syn);
}

// device-resident planar float32 samples; b and hist stay host pointers
extern "C" int ds_rtfir_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_samples, const double* b, int n_taps,
                            const double* hist, float* y, int64_t ld_y) {
    const RtFir f{"ds_rtfir_dev", b, n_taps};
    if (!c || !x || !y) return fail(c, DS_ERR_ARG, f.who, "null argument");
    if (n_ch <= 0 || n_samples <= 0 || ldx < n_samples || ld_y < n_samples) return fail(c, DS_ERR_ARG, f.who, "bad shape");
    CHK(rtfir_check(c, f, n_ch, n_samples));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(mem_check(c, f.who, ((size_t)f.nt4() + (size_t)n_ch * f.order()) * 8 + 2 * 256, 0, 0));
    return rtfir_run<float>(c, f, x, ldx, 1, n_samples, n_ch, hist, y, ld_y, 1);
}

// host pointers: x and y (n_samples, n_ch) float64
extern "C" int ds_rtfir(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, const double* b, int n_taps,
                        const double* hist, double* y) {
    const RtFir f{"ds_rtfir", b, n_taps};
    if (!c || !x || !y) return fail(c, DS_ERR_ARG, f.who, "null argument");
    if (n_ch <= 0 || n_samples <= 0) return fail(c, DS_ERR_ARG, f.who, "bad shape");
    CHK(rtfir_check(c, f, n_ch, n_samples));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nx = (size_t)n_ch * n_samples;
    CHK(mem_check(c, f.who, ((size_t)f.nt4() + (size_t)n_ch * f.order()) * 8 + 2 * 256, 2 * nx * 8, 0));
    return staged(c, {{8, nx, x}, {8, nx, nullptr, y}}, [&](void* const* dv) {
        return rtfir_run<double>(c, f, (const double*)dv[0], 1, n_ch, n_samples, n_ch, hist, (double*)dv[1], 1, n_ch);
    });
}

// Everything ds_rtfilt and ds_rtfilt_dev share.  ldx, ld_y: the _dev entry's row strides (the host entry's rows are dense).
struct RtfiltCall {
    const char* who;
    int n_ch;
    int64_t n_samples, ldx, ld_y;
    int kind, d, aux;
    int64_t delay;
    const double* coef;  // host, packed as kernels_rtfilt.hpp lays it out
    const double* fir;   // host, the FIR part of a parallel filter or nullptr
    int n_fir;
    int64_t n_groups() const { return (n_samples + rtfilt::G - 1) / rtfilt::G; }
    size_t n_coef() const { return (size_t)rtfilt::coef_count(kind, d, aux); }
    RtFir fir_part() const { return RtFir{who, fir, n_fir}; }
    // coefficients, Phi, Phi^B, group states, the padded taps, the FIR part's float64 samples (held when `base_in_ws`):
    // six 256-byte aligned pieces
    size_t ws_bytes(bool base_in_ws) const {
        return (n_coef() + 2 * (size_t)d * d + (size_t)n_ch * (size_t)n_groups() * d + (fir ? (size_t)fir_part().nt4() : 0) +
                (fir && base_in_ws ? (size_t)n_ch * (size_t)n_samples : 0)) * 8 + 6 * 256;
    }
};

// shape and bounds; nothing touches the device
static int rtfilt_check(ds_ctx* c, const RtfiltCall& q, const void* x, const void* y) {
    if (!c || !x || !y || !q.coef) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_ch <= 0 || q.n_samples <= 0 || q.d <= 0 || q.ldx < q.n_samples || q.ld_y < q.n_samples)
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (q.kind < 0 || q.kind >= rtfilt::N_KINDS) return fail(c, DS_ERR_ARG, q.who, "unknown filter kind");
    if (q.d > rtfilt::MAX_D)
        return fail(c, DS_ERR_UNSUP, q.who, "more than 64 states in one filter is not built (the carry's state vector is "
                                            "one value per lane of a wave)");
    if ((q.kind == rtfilt::SVF && q.d != 2) || (q.kind == rtfilt::PARALLEL && (q.aux < 1 || q.d != 2 * q.aux)) ||
        (q.kind != rtfilt::PARALLEL && (q.aux != 0 || q.delay != 0 || q.fir)) || q.delay < 0)
        return fail(c, DS_ERR_ARG, q.who, "the state count, delay or FIR part does not fit the filter kind");
    CHK(carry_limits(c, q.who, q.n_ch, q.n_samples, "more than 65535 channels is not built yet"));
    for (size_t i = 0; i < q.n_coef(); ++i)
        if (!std::isfinite(q.coef[i])) return fail(c, DS_ERR_ARG, q.who, "coefficients must be finite");
    if (q.fir) CHK(rtfir_check(c, q.fir_part(), q.n_ch, q.n_samples));
    if (rtfilt::lds_bytes(q.kind, q.d, true) > 160 * 1024)
        return fail(c, DS_ERR_UNSUP, q.who, "the filter's tiles and states do not fit the 160 KB of local memory");
    return DS_OK;
}

// Host side of the carry, as sfilt_tables: A's column j is one zero-input step of the filter's own step function from the
// unit state e_j; Phi = A^L and Phi^B by squaring; the carry gain is the largest magnitude in the two.
static int rtfilt_tables(ds_ctx* c, const RtfiltCall& q, SfiltTables& tb) {
    const int d = q.d;
    std::vector<double> a((size_t)d * d, 0.0), st((size_t)d), nx((size_t)d);
    for (int j = 0; j < d; ++j) {
        std::fill(st.begin(), st.end(), 0.0);
        st[j] = 1.0;
        rtfilt::step_state_only(q.kind, 0.0, st.data(), nx.data(), q.coef, d, q.aux);
        for (int i = 0; i < d; ++i) a[(size_t)i * d + j] = st[i];
    }
    carry::carry_powers(a, d, tb.phi, tb.phig);
    double gain = 0.0;
    for (const std::vector<double>* m : {&tb.phi, &tb.phig})
        for (double v : *m) gain = std::isfinite(v) ? std::max(gain, std::fabs(v)) : INFINITY;
    if (!(gain <= rtfilt::max_gain(q.kind)))
        return fail(c, DS_ERR_UNSUP, q.who, "the recursion's carry gain (largest magnitude in Phi = A^32 and Phi^64) is "
                                            "above the limit: an unstable or too ill-conditioned filter is not run "
                                            "time-parallel");
    return DS_OK;
}

// the FIR part (if any) and the three passes over device buffers of either sample type; y element (b, c, n) at
// y[b syb + c syc + n syn]; zi, zf: device arrays [D][n_ch] or nullptr.  The FIR part's samples go to a float64 piece of
// c->ws, or, when y is float64 itself (y_as_base), straight into y, where the apply pass adds the sections to them.
template <typename T>
static int rtfilt_run(ds_ctx* c, const RtfiltCall& q, const SfiltTables& tb, const T* x, int64_t sxc, int64_t sxn,
                      const double* zi, T* y, int64_t syb, int64_t syc, int64_t syn, double* zf, bool y_as_base) {
    const int d = q.d, n_ch = q.n_ch;
    const int64_t n = q.n_samples, n_groups = q.n_groups();
    const RtFir f = q.fir_part();
    const std::vector<double> taps = q.fir ? f.padded() : std::vector<double>();
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, q.n_coef(), q.coef}, {8, tb.phi.size(), tb.phi.data()},
                                        {8, tb.phig.size(), tb.phig.data()}, {8, (size_t)n_ch * n_groups * d},
                                        {8, taps.size(), taps.data()},
                                        {8, q.fir && !y_as_base ? (size_t)n_ch * (size_t)n : 0}}, t));
    const double *dcoef = (const double*)t[0], *dphi = (const double*)t[1], *dphig = (const double*)t[2];
    double* gst = (double*)t[3];
    const double* base = nullptr;
    int64_t sbc = 0, sbn = 0;
    if (q.fir) {
        if constexpr (std::is_same<T, double>::value) {
            if (y_as_base) {
                CHK((rtfir_launch<T, double>(c, f, x, sxc, sxn, n, n_ch, (const double*)t[4], nullptr, y, syc, syn)));
                base = y, sbc = syc, sbn = syn;
            }
        }
        if (!base) {
            CHK((rtfir_launch<T, double>(c, f, x, sxc, sxn, n, n_ch, (const double*)t[4], nullptr, (double*)t[5], n, 1)));
            base = (const double*)t[5], sbc = n, sbn = 1;
        }
    }
    rtfilt::Args<T> a{x, sxc, sxn, y, syb, syc, syn, n, n_ch, q.kind, d, q.aux, n_groups, q.delay, base, sbc, sbn,
                      dcoef, dphi, dphig, gst, zi, zf};
    if (n_groups > 1)
        CHK(launch(c, "rtfilt_group", rtfilt::k_rtfilt_group<T>, dim3((unsigned)(n_groups - 1), (unsigned)n_ch), rtfilt::B,
                   rtfilt::lds_bytes(q.kind, d, false), a));
    carry::CarryArgs ca{dphig, gst, zi, n_groups, n_ch, d};  // one filter: zi [D][n_ch]
    CHK(launch(c, "rtfilt_carry", carry::k_block_carry, dim3((unsigned)n_ch), rtfilt::B, sizeof(double) * d * d, ca));
    return launch(c, "rtfilt_apply", rtfilt::k_rtfilt_apply<T>, dim3((unsigned)n_groups, (unsigned)n_ch), rtfilt::B,
                  rtfilt::lds_bytes(q.kind, d, true), a);
}

// device-resident planar float32 samples; coef, fir, zi and zf stay host pointers (zi / zf [D][n_ch] cross through c->io);
// band b of channel c at y[(b n_ch + c) ld_y + n]
extern "C" int ds_rtfilt_dev(ds_ctx* c, const float* x, int n_ch, int64_t ldx, int64_t n_samples, int kind,
                             const double* coef, int d, int aux, int64_t delay, const double* fir, int n_fir,
                             const double* zi, float* y, int64_t ld_y, double* zf) {
    const RtfiltCall q{"ds_rtfilt_dev", n_ch, n_samples, ldx, ld_y, kind, d, aux, delay, coef, n_fir > 0 ? fir : nullptr, n_fir};
    if (n_fir > 0 && !fir) return fail(c, DS_ERR_ARG, q.who, "null argument");
    CHK(rtfilt_check(c, q, x, y));
    SfiltTables tb;
    CHK(rtfilt_tables(c, q, tb));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nz = (size_t)d * n_ch;
    CHK(mem_check(c, q.who, q.ws_bytes(true), 2 * nz * 8, 0));
    return staged(c, {{8, nz, zi}, {8, zf ? nz : 0, nullptr, zf}}, [&](void* const* dv) {
        return rtfilt_run<float>(c, q, tb, x, ldx, 1, zi ? (const double*)dv[0] : nullptr, y, (int64_t)n_ch * ld_y, ld_y, 1,
                                 zf ? (double*)dv[1] : nullptr, false);
    });
}

// host pointers in the reference's layouts: x (n_samples, n_ch) and y (bands, n_samples, n_ch) float64, bands = 4 for the
// state-variable filter and 1 otherwise
extern "C" int ds_rtfilt(ds_ctx* c, const double* x, int n_ch, int64_t n_samples, int kind, const double* coef, int d,
                         int aux, int64_t delay, const double* fir, int n_fir, const double* zi, double* y, double* zf) {
    const RtfiltCall q{"ds_rtfilt", n_ch, n_samples, n_samples, n_samples, kind, d, aux, delay, coef, n_fir > 0 ? fir : nullptr, n_fir};
    if (n_fir > 0 && !fir) return fail(c, DS_ERR_ARG, q.who, "null argument");
    CHK(rtfilt_check(c, q, x, y));
    SfiltTables tb;
    CHK(rtfilt_tables(c, q, tb));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nx = (size_t)n_ch * n_samples, ny = nx * rtfilt::n_bands(kind), nz = (size_t)d * n_ch;
    CHK(mem_check(c, q.who, q.ws_bytes(false), (nx + ny + 2 * nz) * 8, 0));
    return staged(c, {{8, nx, x}, {8, ny, nullptr, y}, {8, nz, zi}, {8, zf ? nz : 0, nullptr, zf}}, [&](void* const* dv) {
        return rtfilt_run<double>(c, q, tb, (const double*)dv[0], 1, n_ch, zi ? (const double*)dv[2] : nullptr,
                                  (double*)dv[1], (int64_t)nx, 1, n_ch, zf ? (double*)dv[3] : nullptr, true);
    });
}

// ---- shoebox room simulation (kernels_room.hpp), float64 ----------------------------------------------------------
// pw: host (n_band, 6, limit + 2); out: host (n_band, n_out)
extern "C" int ds_room_ism(ds_ctx* c, const double dim[3], const double src[3], const double rec[3], double sr, double cs,
                           int limit, const double* pw, int n_band, int64_t n_out, int64_t max_list_bytes, double* out) {
    using namespace dsroom;
    const char* who = "ds_room_ism";
    if (!c || !dim || !src || !rec || !pw || !out) return fail(c, DS_ERR_ARG, who, "null argument");
    if (limit < 0 || n_band < 1 || n_out < 1 || !(sr > 0) || !(cs > 0) || !std::isfinite(sr) || !std::isfinite(cs))
        return fail(c, DS_ERR_ARG, who, "needs limit >= 0, bands, output samples and positive finite sr and c");
    for (int a = 0; a < 3; ++a)
        if (!(dim[a] > 0) || !std::isfinite(dim[a]) || !std::isfinite(src[a]) || !std::isfinite(rec[a]))
            return fail(c, DS_ERR_ARG, who, "needs positive finite dimensions and finite positions");
    if (ism_shape_unsupported(limit, n_out, n_band))
        return fail(c, DS_ERR_UNSUP, who, "more than 2^27 cells, 2^24 output samples or 8 bands are not built");
    if (max_list_bytes <= 0 || max_list_bytes > kIsmMaxListBytes) max_list_bytes = kIsmMaxListBytes;
    const int64_t side = 2 * (int64_t)limit + 1, planes = ism_slab_planes(limit, max_list_bytes);
    if (planes < 1) return fail(c, DS_ERR_UNSUP, who, "the id list does not hold one l plane of sources");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_pw = (size_t)n_band * 6 * (limit + 2), n_y = (size_t)n_band * n_out, n_cnt = (size_t)n_out + 1;
    const size_t n_list = (size_t)planes * side * side * 8;
    CHK(mem_check(c, who, 2 * n_cnt * 4 + n_list * 4, (n_pw + n_y) * 8, 0));
    uint32_t *count, *cursor, *list;
    CHK(carve(c, &c->ws, &c->ws_bytes, [&](Carver& cv) {
        count = cv.take<uint32_t>(n_cnt);
        cursor = cv.take<uint32_t>(n_cnt);
        list = cv.take<uint32_t>(n_list);
    }));
    return staged(c, {{8, n_pw, pw, nullptr}, {8, n_y, nullptr, out}}, [&](void* const* d) {
        IsmArgs a{};
        for (int k = 0; k < 3; ++k) a.dim[k] = dim[k], a.s[k] = src[k], a.r[k] = rec[k];
        a.c = cs, a.sr = sr, a.limit = limit, a.n_out = n_out, a.n_band = n_band;
        a.pw = (const double*)d[0], a.count = count, a.cursor = cursor, a.list = list, a.out = (double*)d[1];
        CHK(ds_memset(c, a.out, 0, n_y * 8));
        // slabs in ascending l: k_ism_sum continues the sums the earlier slabs left, so the additions keep their order
        for (int64_t l0 = 0; l0 < side; l0 += planes) {
            a.l0 = (int)l0, a.l1 = (int)std::min(l0 + planes, side);
            const int64_t cells = (int64_t)(a.l1 - a.l0) * side * side;
            const dim3 grid((unsigned)((cells + NT - 1) / NT));
            CHK(ds_memset(c, count, 0, n_cnt * 4));
            CHK(launch(c, "room_ism_count", k_ism_count, grid, NT, 0, a));
            CHK(launch(c, "room_ism_scan", k_ism_scan, dim3(1), SCAN_NT, 0, a));
            CHK(launch(c, "room_ism_fill", k_ism_fill, grid, NT, 0, a));
            CHK(launch(c, "room_ism_sum", k_ism_sum, dim3((unsigned)n_out), NT, 0, a));
        }
        return DS_OK;
    });
}

// omega_n, eta, weight: host (n_modes); omega2: host (n_freq); p: host (n_freq) complex128
extern "C" int ds_room_modal_tf(ds_ctx* c, const double* omega_n, const double* eta, const double* weight, int64_t n_modes,
                                const double* omega2, int64_t n_freq, double* p) {
    using namespace dsroom;
    const char* who = "ds_room_modal_tf";
    if (n_modes < 1 || n_freq < 1) return fail(c, DS_ERR_ARG, who, "needs a mode and a frequency");
    if (n_freq > ((int64_t)1 << 31) - 1 || modal_work_too_large(n_modes, n_freq))
        return fail(c, DS_ERR_UNSUP, who, "modes x frequencies is beyond the work bound");
    if (!c || !omega_n || !eta || !weight || !omega2 || !p) return fail(c, DS_ERR_ARG, who, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nm = (size_t)n_modes, nf = (size_t)n_freq;
    CHK(mem_check(c, who, 0, (3 * nm + 3 * nf) * 8, 0));
    return staged(c, {{8, nm, omega_n, nullptr}, {8, nm, eta, nullptr}, {8, nm, weight, nullptr}, {8, nf, omega2, nullptr},
                      {16, nf, nullptr, p}}, [&](void* const* d) {
        return launch(c, "room_modal_tf", k_modal_tf, dim3((unsigned)((nf + MODAL_NT - 1) / MODAL_NT)), MODAL_NT, 0,
                      ModalArgs{(const double*)d[0], (const double*)d[1], (const double*)d[2], n_modes,
                                (const double*)d[3], n_freq, (double2*)d[4]});
    });
}

// ---- variable-Q transform and its integer-ratio resampler (kernels_vqt.hpp) --------------------------------------------
// taps of scipy's default resample_poly filter for the rate r; a rate of 1 is the one-tap copy
static int vqt_rate_taps(int r) { return r == 1 ? 1 : 20 * r + 1; }

// P(x, 1, D): sample n of channel ch at x[n ss + ch cs] -> out (n_out, n_ch) float64; h: device, vqt_rate_taps(D) taps
template <typename T>
static int vqt_decimate(ds_ctx* c, const T* x, int64_t ss, int64_t cs, int64_t n_in, int n_ch, const double* h, int D,
                        double* out, int64_t n_out) {
    using namespace dsvqt;
    const int cg = ch_group(n_ch), dt = NT / cg, ntaps = vqt_rate_taps(D);
    return launch(c, "vqt_decimate", k_vqt_decimate<T>, dim3((unsigned)((n_out + dt - 1) / dt), (unsigned)((n_ch + cg - 1) / cg)),
                  NT, dec_lds_doubles(ntaps, D, cg) * 8, DecArgs<T>{x, ss, cs, n_in, n_ch, cg, h, ntaps, D, out, n_out});
}

// One interpolation launch over the octaves oc[0 .. n_e) (a device table; host_oc its host copy), `rows` rows each.
template <typename V>
static int vqt_interp(ds_ctx* c, const char* name, const V* in, V* out, const double* taps, const dsvqt::InterpOct* oc,
                      const dsvqt::InterpOct* host_oc, int n_e, int rows, int n_ch) {
    using namespace dsvqt;
    const int cg = ch_group(n_ch);
    int64_t tiles = 0;
    size_t lds = 0;
    for (int e = 0; e < n_e; ++e) {  // (the octaves of one launch share HW: every rate is above 1, or it is d = 1)
        const int64_t tile = (int64_t)interp_span((int)host_oc[e].U, cg) * host_oc[e].U;
        tiles = std::max(tiles, (host_oc[e].n_out + tile - 1) / tile);
        lds = std::max(lds, interp_lds_bytes((int)host_oc[e].U, (int)host_oc[e].HW, cg, sizeof(V)));
    }
    if (tiles < 1) return DS_OK;
    if (tiles > INT32_MAX) return fail(c, DS_ERR_UNSUP, "vqt: more sample tiles than one launch covers");
    const dim3 grid((unsigned)tiles, (unsigned)((n_ch + cg - 1) / cg), (unsigned)(n_e * rows));
    const InterpArgs<V> a{in, out, taps, oc, n_ch, cg, rows};
    if (host_oc[0].HW == 0) return launch(c, name, k_vqt_interp<V, 0>, grid, NT, lds, a);
    return launch(c, name, k_vqt_interp<V, 10>, grid, NT, lds, a);
}

struct VqtCall {
    const char* who;
    int64_t n_samples;
    int n_ch, d, n_oct, bins;
    const int64_t* kernel_len;
    const double *kernel_taps, *taps_dec, *taps_half, *taps_up;
};

// x: the samples on the device (T = double: interleaved, staged by the entry; T = float: planar where they lie);
// out: the device's (n_oct bins, n_samples, n_ch) complex128 result
template <typename T>
static int vqt_run(ds_ctx* c, const VqtCall& q, const T* x, int64_t ss, int64_t cs, double2* out) {
    using namespace dsvqt;
    const int C = q.n_ch, bins = q.bins, n_oct = q.n_oct, F = n_oct * bins;
    const int64_t N = q.n_samples;
    // octave lengths: len(td_0) = ceil(N / d), then halved (rounding up) per octave.  len(td_o) 2^o >= len(td_0) and
    // len(td_0) d >= N, so every interpolated row reaches N samples: the reference's zero-padding branch is never taken
    // and is not built.
    int64_t M[MAX_OCT], td_off[MAX_OCT], z_off[MAX_OCT], y_off[MAX_OCT], n_td = 0, n_z = 0, n_y = 0;
    for (int o = 0; o < n_oct; ++o) {
        M[o] = o == 0 ? (N + q.d - 1) / q.d : (M[o - 1] + 1) / 2;
        td_off[o] = n_td;
        z_off[o] = n_z;
        y_off[o] = n_y;
        n_td += M[o] * C;
        n_z += (int64_t)bins * M[o] * C;
        if (o > 0) n_y += (int64_t)bins * (M[o] << o) * C;
    }
    // the tables of the launches: the kernels' (first tap, length), the bank's octaves, the two interpolation stages'
    std::vector<int64_t> kdesc(2 * (size_t)bins);
    int64_t n_ktaps = 0, lmax = 0;
    for (int i = 0; i < bins; ++i) {
        kdesc[2 * i] = n_ktaps;
        kdesc[2 * i + 1] = q.kernel_len[i];
        n_ktaps += q.kernel_len[i];
        lmax = std::max(lmax, q.kernel_len[i]);
    }
    std::vector<BankOct> boct(n_oct);
    std::vector<InterpOct> first, last(n_oct);
    int64_t up_off = 0;
    for (int o = 0; o < n_oct; ++o) {
        boct[o] = BankOct{td_off[o], z_off[o], M[o]};
        if (o > 0) {
            first.push_back(InterpOct{z_off[o], M[o], y_off[o], M[o] << o, 0, 1, up_off, (int64_t)1 << o, 10});
            up_off += vqt_rate_taps(1 << o);
        }
    }
    for (int o = 0; o < n_oct; ++o)  // octave 0 is read from the bank's rows, the others from the first stage's
        last[o] = InterpOct{o == 0 ? z_off[0] : n_z + y_off[o], M[o] << o, 0, N, F - 1 - (int64_t)o * bins, -1, up_off, q.d,
                            q.d == 1 ? 0 : 10};
    const size_t n_up = (size_t)up_off + vqt_rate_taps(q.d), n_first = first.size();
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, kdesc.size(), kdesc.data()}, {sizeof(BankOct), (size_t)n_oct, boct.data()},
                                        {sizeof(InterpOct), n_first, first.data()}, {sizeof(InterpOct), (size_t)n_oct, last.data()},
                                        {16, (size_t)n_ktaps, q.kernel_taps}, {8, (size_t)vqt_rate_taps(q.d), q.taps_dec},
                                        {8, (size_t)vqt_rate_taps(2), q.taps_half}, {8, n_up, q.taps_up}, {8, (size_t)n_td},
                                        {16, (size_t)(n_z + n_y)}}, t));
    const double *h_dec = (const double*)t[5], *h_half = (const double*)t[6], *h_up = (const double*)t[7];
    double* td = (double*)t[8];
    double2* zy = (double2*)t[9];  // the bank's rows of every octave, then the first stage's
    CHK(vqt_decimate<T>(c, x, ss, cs, N, C, h_dec, q.d, td, M[0]));
    for (int o = 1; o < n_oct; ++o)
        CHK(vqt_decimate<double>(c, td + td_off[o - 1], C, 1, M[o - 1], C, h_half, 2, td + td_off[o], M[o]));
    const int cg = ch_group(C), bt = NT / cg;
    CHK(launch(c, "vqt_bank", k_vqt_bank, dim3((unsigned)((M[0] + bt - 1) / bt), (unsigned)((C + cg - 1) / cg), (unsigned)F), NT,
               bank_lds_bytes((int)lmax, cg),
               BankArgs{td, (const BankOct*)t[1], (const int64_t*)t[0], (const double2*)t[4], zy, C, cg, bins}));
    if (n_first)
        CHK(vqt_interp<double2>(c, "vqt_interp_octave", zy, zy + n_z, h_up, (const InterpOct*)t[2], first.data(), (int)n_first,
                                bins, C));
    return vqt_interp<double2>(c, "vqt_interp", zy, out, h_up, (const InterpOct*)t[3], last.data(), n_oct, bins, C);
}

extern "C" int ds_vqt(ds_ctx* c, const void* x, int x_on_device, int n_ch, int64_t ldx, int64_t n_samples, int d, int n_oct,
                      int bins, const int64_t* kernel_len, const double* kernel_taps, const double* taps_dec,
                      const double* taps_half, const double* taps_up, void* out, int out_on_device) {
    const char* who = "ds_vqt";
    if (!c || !x || !out || !kernel_len || !kernel_taps || !taps_dec || !taps_half || !taps_up)
        return fail(c, DS_ERR_ARG, who, "null argument");
    if (n_samples < 1 || n_ch < 1 || d < 1 || n_oct < 1 || bins < 1 || (x_on_device && ldx < n_samples))
        return fail(c, DS_ERR_ARG, who, "bad shape");
    int64_t lmax = 0;
    for (int i = 0; i < bins; ++i) {
        if (kernel_len[i] < 1) return fail(c, DS_ERR_ARG, who, "a kernel has no taps");
        lmax = std::max(lmax, kernel_len[i]);
    }
    const int64_t rows = (int64_t)n_oct * bins;
    if (vqt_shape_unsupported(d, n_oct, lmax, rows, n_ch))
        return fail(c, DS_ERR_UNSUP, who, "beyond d <= 48, octaves <= 7, kernels of 2048 taps or 65535 rows or channel groups");
    if (vqt_output_too_large(rows, n_samples, n_ch)) return fail(c, DS_ERR_UNSUP, who, "the result is larger than 2^34 bytes");
    HIPCHK(c, hipSetDevice(c->device));
    const VqtCall q{who, n_samples, n_ch, d, n_oct, bins, kernel_len, kernel_taps, taps_dec, taps_half, taps_up};
    const size_t n_x = x_on_device ? 0 : (size_t)n_samples * n_ch, n_out = out_on_device ? 0 : (size_t)rows * n_samples * n_ch;
    // the workspace: the decimated samples (at most 2 (N / d + 2) C), the bank's rows (twice that per bin) and the first
    // stage's (N / d + 64 per row)
    const size_t m0 = (size_t)((n_samples + d - 1) / d) + 2;
    CHK(mem_check(c, who, 16 * m0 * n_ch + 32 * (size_t)rows * (m0 + 64) * n_ch + ((size_t)1 << 20), (n_x * 8 + n_out * 16), 0));
    return staged(c, {{8, n_x, x}, {16, n_out, nullptr, out_on_device ? nullptr : out}}, [&](void* const* s) {
        double2* dout = out_on_device ? (double2*)out : (double2*)s[1];
        if (x_on_device) return vqt_run<float>(c, q, (const float*)x, 1, ldx, dout);
        return vqt_run<double>(c, q, (const double*)s[0], n_ch, 1, dout);
    });
}

extern "C" int ds_resample_int(ds_ctx* c, const double* x, int64_t n, int n_ch, int up, int down, const double* taps,
                               double* out) {
    using namespace dsvqt;
    const char* who = "ds_resample_int";
    if (!c || !x || !taps || !out) return fail(c, DS_ERR_ARG, who, "null argument");
    if (n < 1 || n_ch < 1 || up < 1 || down < 1 || (up != 1 && down != 1))
        return fail(c, DS_ERR_ARG, who, "needs samples, channels and an integer ratio: one of up and down is 1");
    if (down > kVqtMaxDecimation || up > (1 << (kVqtMaxOctaves - 1)) || (n_ch + 3) / 4 > kVqtMaxRows)
        return fail(c, DS_ERR_UNSUP, who, "beyond down <= 48, up <= 64 or 65535 channel groups");
    const int64_t n_out = down == 1 ? n * up : (n + down - 1) / down;
    if ((double)n_out * n_ch * 8.0 > (double)kVqtMaxOutputBytes) return fail(c, DS_ERR_UNSUP, who, "the result is larger than 2^34 bytes");
    HIPCHK(c, hipSetDevice(c->device));
    const int r = std::max(up, down);
    const InterpOct oc{0, n, 0, n_out, 0, 1, 0, up, up == 1 ? 0 : 10};
    return staged(c, {{8, (size_t)n * n_ch, x}, {8, (size_t)n_out * n_ch, nullptr, out}}, [&](void* const* s) {
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, (size_t)vqt_rate_taps(r), taps}, {sizeof(InterpOct), 1, &oc}}, t));
        if (down > 1) return vqt_decimate<double>(c, (const double*)s[0], n_ch, 1, n, n_ch, (const double*)t[0], down, (double*)s[1], n_out);
        return vqt_interp<double>(c, "vqt_interp@real", (const double*)s[0], (double*)s[1], (const double*)t[0],
                                  (const InterpOct*)t[1], &oc, 1, 1, n_ch);
    });
}

// ---- rational-ratio resampling (kernels_resample.hpp, resample_plan.hpp), float64 arithmetic ---------------------------
static_assert(resample::MAX_RATE == kResampleMaxRate, "the plan and the guard name the same rate");

struct ResampleCall {
    const char* who;
    int64_t n;
    int n_ch, up, down;
    const double* taps;  // host, up * firwin(20 r + 1, 1 / r, kaiser 5.0) with r = max(up, down)
    int64_t n_out() const { return resample::out_len(n, up, down); }
};

// shape and bounds; nothing touches the device
static int resample_check(ds_ctx* c, const ResampleCall& q, const void* x, const void* y) {
    if (!x || !y || !q.taps) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n < 1 || q.n_ch < 1 || q.up < 1 || q.down < 1 || (q.up == 1 && q.down == 1) || std::gcd(q.up, q.down) != 1)
        return fail(c, DS_ERR_ARG, q.who, "needs samples, channels and a reduced ratio other than 1 / 1");
    if (resample_shape_unsupported(q.up, q.down, q.n, q.n_out(), q.n_ch))
        return fail(c, DS_ERR_UNSUP, q.who, "a rate beyond 640, more than 2^31 samples in all or more than 65535 channels are not built");
    if (!c) return fail(c, DS_ERR_ARG, q.who, "null argument");
    return DS_OK;
}

// sample n of channel ch at x[n xss + ch xcs] -> y[m yss + ch ycs], both on the device
template <typename TI, typename TO>
static int resample_run(ds_ctx* c, const ResampleCall& q, const TI* x, int64_t xss, int64_t xcs, TO* y, int64_t yss, int64_t ycs) {
    namespace rs = resample;
    const rs::Plan pl = rs::make_plan(q.up, q.down, q.n_ch);
    std::vector<double> hp((size_t)rs::table_doubles(pl));
    rs::phase_major(pl, q.taps, hp.data());
    void* t[kMaxStaged];
    CHK(stage(c, &c->ws, &c->ws_bytes, {{8, hp.size(), hp.data()}}, t));
    const int64_t n_out = q.n_out(), tiles = (n_out + pl.tile - 1) / pl.tile;
    if (tiles > INT32_MAX) return fail(c, DS_ERR_UNSUP, q.who, "more tiles than one launch covers");
    return launch(c, "resample_poly", rs::k_resample_poly<TI, TO>, dim3((unsigned)tiles, (unsigned)((q.n_ch + pl.cg - 1) / pl.cg)),
                  rs::NT, (size_t)rs::lds_doubles(pl) * 8,
                  rs::PolyArgs<TI, TO>{x, xss, xcs, q.n, (const double*)t[0], y, yss, ycs, n_out, q.n_ch, pl});
}

// x: host (n, n_ch) float64 -> out: host (ceil(n up / down), n_ch) float64
extern "C" int ds_resample_poly(ds_ctx* c, const double* x, int64_t n, int n_ch, int up, int down, const double* taps,
                                double* out) {
    const ResampleCall q{"ds_resample_poly", n, n_ch, up, down, taps};
    CHK(resample_check(c, q, x, out));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nx = (size_t)n * n_ch, ny = (size_t)q.n_out() * n_ch;
    CHK(mem_check(c, q.who, (size_t)resample::LDS_DOUBLES * 8, (nx + ny) * 8, 0));
    return staged(c, {{8, nx, x}, {8, ny, nullptr, out}}, [&](void* const* d) {
        return resample_run<double, double>(c, q, (const double*)d[0], n_ch, 1, (double*)d[1], n_ch, 1);
    });
}

// x: planar float32 on the device, channel ch at x + ch ldx -> y: planar float32 on the device, channel ch at y + ch ld_y
extern "C" int ds_resample_poly_dev(ds_ctx* c, const float* x, int64_t ldx, int64_t n, int n_ch, int up, int down,
                                    const double* taps, float* y, int64_t ld_y) {
    const ResampleCall q{"ds_resample_poly_dev", n, n_ch, up, down, taps};
    CHK(resample_check(c, q, x, y));
    if (ldx < n || ld_y < q.n_out()) return fail(c, DS_ERR_ARG, q.who, "bad shape");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(mem_check(c, q.who, (size_t)resample::LDS_DOUBLES * 8, 0, 0));
    return resample_run<float, float>(c, q, x, 1, ldx, y, 1, ld_y);
}

// ---- audio effects (kernels_fx.hpp), float64 ------------------------------------------------------------------------
// What every effects entry takes: x (n samples of n_str streams) and y (n_out samples) both on the host as
// (samples, streams) float64, or both on the device as planar float32 rows of pitch ldx / ld_y.
struct FxCall {
    const char* who;
    const void* x;
    int on_device, n_str;
    int64_t ldx, n, n_out;
    void* y;
    int64_t ld_y;
    size_t elements() const { return (size_t)n_str * (size_t)n_out; }
};

// shape and bounds; nothing touches the device
static int fx_check(ds_ctx* c, const FxCall& q) {
    if (!c || !q.x || !q.y) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_str < 1 || q.n < 1 || q.n_out < q.n || (q.on_device && (q.ldx < q.n || q.ld_y < q.n_out)))
        return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (fx_shape_unsupported(q.n_str, q.n_out))
        return fail(c, DS_ERR_UNSUP, q.who, "more than 65535 streams, 2^28 samples a stream or 2^30 samples in all are not built");
    return DS_OK;
}

// run(src, dst) over the samples where they lie: a host call's arrays are pieces of c->io, a resident call's are read
// and written in place.  ws_doubles: what run() will carve out of c->ws, for the memory pre-check.
template <class F>
static int fx_io(ds_ctx* c, const FxCall& q, size_t ws_doubles, F&& run) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nx = q.on_device ? 0 : (size_t)q.n_str * q.n, ny = q.on_device ? 0 : q.elements();
    CHK(mem_check(c, q.who, ws_doubles * 8 + 16 * 256, (nx + ny) * 8, 0));
    if (q.on_device)
        return run(dsfx::Src<float>{(const float*)q.x, 1, q.ldx}, dsfx::Dst<float>{(float*)q.y, 1, q.ld_y});
    return staged(c, {{8, nx, q.x}, {8, ny, nullptr, q.y}}, [&](void* const* d) {
        return run(dsfx::Src<double>{(const double*)d[0], q.n_str, 1}, dsfx::Dst<double>{(double*)d[1], q.n_str, 1});
    });
}

static dim3 fx_grid(int64_t n, int n_str) { return dim3((unsigned)((n + dsfx::NT - 1) / dsfx::NT), (unsigned)n_str); }

template <typename T>
static int fx_stats(ds_ctx* c, dsfx::Src<T> x, int64_t n, int n_str, double gain, double* st) {
    return launch(c, "fx_stats", dsfx::k_fx_stats<T>, dim3((unsigned)n_str), dsfx::STATS_NT, 0, dsfx::StatsArgs<T>{x, n, gain, st});
}

// the restore stage of compressor, delay and chorus: yd [n_str][n] -> dst
template <typename T>
static int fx_scale(ds_ctx* c, const double* yd, dsfx::Dst<T> y, int64_t n, int n_str, int restore, const double* st_in,
                    double* st_out, double gain) {
    if (restore != dsfx::RESTORE_NONE) CHK(fx_stats(c, dsfx::Src<double>{yd, 1, n}, n, n_str, 1.0, st_out));
    return launch(c, "fx_scale", dsfx::k_fx_scale<T>, fx_grid(n, n_str), dsfx::NT, 0,
                  dsfx::ScaleArgs<T>{yd, y, n, restore, st_in, st_out, gain});
}

// par: gain_pre, threshold_db, ratio, knee_db, c_attack, c_release, min_power, gain_post
extern "C" int ds_fx_compress(ds_ctx* c, const void* x, int on_device, int n_str, int64_t ldx, int64_t n, const double* par,
                              int downward, int relative, int make_up, void* y, int64_t ld_y) {
    const FxCall q{"ds_fx_compress", x, on_device, n_str, ldx, n, n, y, ld_y};
    CHK(fx_check(c, q));
    if (!par) return fail(c, DS_ERR_ARG, q.who, "null argument");
    const dsfx::FollowPar p{par[0], par[1], par[2], par[3], par[4], par[5], par[6], downward, relative};
    const size_t n_st = (size_t)n_str * dsfx::STAT;
    return fx_io(c, q, 2 * n_st + q.elements(), [&](auto src, auto dst) {
        using T = typename decltype(src)::type;
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, n_st}, {8, n_st}, {8, q.elements()}}, t));
        double *st_in = (double*)t[0], *st_out = (double*)t[1], *yd = (double*)t[2];
        CHK(fx_stats(c, src, n, n_str, p.gain, st_in));
        CHK(launch(c, "fx_follow@compress", dsfx::k_fx_follow<T, dsfx::MODE_COMPRESS>, dim3((unsigned)n_str), dsfx::FOLLOW_NT, 0,
                   dsfx::FollowArgs<T>{src, n, p, st_in, yd, nullptr}));
        return fx_scale(c, yd, dst, n, n_str, make_up ? dsfx::RESTORE_RMS : dsfx::RESTORE_NONE, st_in, st_out, par[7]);
    });
}

// mask: host (n_str, n) bytes, 1 where 10 log10(gain) > threshold_db
extern "C" int ds_fx_detect(ds_ctx* c, const void* x, int on_device, int n_str, int64_t ldx, int64_t n, double c_release,
                            double threshold_db, int relative, uint8_t* mask) {
    const FxCall q{"ds_fx_detect", x, on_device, n_str, ldx, n, n, mask, n};
    CHK(fx_check(c, q));
    HIPCHK(c, hipSetDevice(c->device));
    const dsfx::FollowPar p{1.0, threshold_db, 1.0, 0.0, 0.0, c_release, 0.0, 1, relative};
    const size_t n_st = (size_t)n_str * dsfx::STAT, nx = on_device ? 0 : q.elements();
    CHK(mem_check(c, q.who, n_st * 8 + 256, nx * 8 + q.elements(), 0));
    return staged(c, {{8, nx, x}, {1, q.elements(), nullptr, mask}}, [&](void* const* d) {
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, n_st}}, t));
        double* st = (double*)t[0];
        auto run = [&](auto src) {
            using T = typename decltype(src)::type;
            CHK(fx_stats(c, src, n, n_str, 1.0, st));
            return launch(c, "fx_follow@detect", dsfx::k_fx_follow<T, dsfx::MODE_DETECT>, dim3((unsigned)n_str), dsfx::FOLLOW_NT, 0,
                          dsfx::FollowArgs<T>{src, n, p, st, nullptr, (uint8_t*)d[1]});
        };
        if (on_device) return run(dsfx::Src<float>{(const float*)x, 1, ldx});
        return run(dsfx::Src<double>{(const double*)d[0], n_str, 1});
    });
}

// y holds n + padding samples a stream
extern "C" int ds_fx_delay(ds_ctx* c, const void* x, int on_device, int n_str, int64_t ldx, int64_t n, int64_t delay,
                           int64_t padding, double feedback, int saturation, void* y, int64_t ld_y) {
    const FxCall q{"ds_fx_delay", x, on_device, n_str, ldx, n, n + std::max<int64_t>(padding, 0), y, ld_y};
    if (delay < 0 || padding < 0 || (delay == 0 && padding != 0) || (saturation != dsfx::SAT_DIGITAL && saturation != dsfx::SAT_ARCTAN))
        return fail(c, DS_ERR_ARG, q.who, "needs delay >= 0, padding >= 0 (0 with no delay) and a known saturation");
    CHK(fx_check(c, q));
    const size_t n_st = (size_t)n_str * dsfx::STAT;
    return fx_io(c, q, 2 * n_st + q.elements(), [&](auto src, auto dst) {
        using T = typename decltype(src)::type;
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, n_st}, {8, n_st}, {8, q.elements()}}, t));
        double *st_in = (double*)t[0], *st_out = (double*)t[1], *yd = (double*)t[2];
        CHK(fx_stats(c, src, n, n_str, 1.0, st_in));
        CHK(launch(c, "fx_comb", dsfx::k_fx_comb<T>, fx_grid(delay ? std::min(delay, q.n_out) : q.n_out, n_str), dsfx::NT, 0,
                   dsfx::CombArgs<T>{src, n, q.n_out, delay, feedback, saturation, yd}));
        return fx_scale(c, yd, dst, q.n_out, n_str, dsfx::RESTORE_PEAK, st_in, st_out, 1.0);
    });
}

// m: host (n, voices) int32, every |m| <= max_delay
extern "C" int ds_fx_chorus(ds_ctx* c, const void* x, int on_device, int n_str, int64_t ldx, int64_t n, const int32_t* m,
                            int voices, int64_t max_delay, double mix, void* y, int64_t ld_y) {
    const FxCall q{"ds_fx_chorus", x, on_device, n_str, ldx, n, n, y, ld_y};
    CHK(fx_check(c, q));
    if (!m) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (voices < 1 || max_delay < 0) return fail(c, DS_ERR_ARG, q.who, "needs a voice and a largest delay >= 0");
    if (voices > kFxMaxVoices || n + max_delay > kFxMaxSamples)
        return fail(c, DS_ERR_UNSUP, q.who, "more than 64 voices or 2^28 padded samples are not built");
    const size_t n_m = (size_t)n * voices;
    for (size_t i = 0; i < n_m; ++i)
        if (m[i] > max_delay || m[i] < -max_delay) return fail(c, DS_ERR_ARG, q.who, "a delay is beyond max_delay");
    const size_t n_st = (size_t)n_str * dsfx::STAT;
    return fx_io(c, q, 2 * n_st + q.elements() + n_m / 2 + 1, [&](auto src, auto dst) {
        using T = typename decltype(src)::type;
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, n_st}, {8, n_st}, {8, q.elements()}, {4, n_m, m}}, t));
        double *st_in = (double*)t[0], *st_out = (double*)t[1], *yd = (double*)t[2];
        CHK(fx_stats(c, src, n, n_str, 1.0, st_in));
        CHK(launch(c, "fx_voices", dsfx::k_fx_voices<T>, fx_grid(n, n_str), dsfx::NT, 0,
                   dsfx::VoicesArgs<T>{src, n, n + max_delay, (const int32_t*)t[3], voices, mix, 1 - mix, yd}));
        return fx_scale(c, yd, dst, n, n_str, dsfx::RESTORE_PEAK, st_in, st_out, 1.0);
    });
}

// kinds [n_curves]: DS_FX_CURVE_*; par [n_curves][3]: linear level, linear offset, mix weight (none of them 0)
extern "C" int ds_fx_distort(ds_ctx* c, const void* x, int on_device, int n_str, int64_t ldx, int64_t n, int n_curves,
                             const int* kinds, const double* par, double gain, void* y, int64_t ld_y) {
    const FxCall q{"ds_fx_distort", x, on_device, n_str, ldx, n, n, y, ld_y};
    CHK(fx_check(c, q));
    if (!kinds || !par || n_curves < 1) return fail(c, DS_ERR_ARG, q.who, "needs a curve");
    if (n_curves > kFxMaxCurves) return fail(c, DS_ERR_UNSUP, q.who, "more than 8 curves are not built");
    dsfx::CurvePar cv{};
    cv.count = n_curves;
    for (int k = 0; k < n_curves; ++k) {
        if (kinds[k] < 0 || kinds[k] >= dsfx::N_CURVES) return fail(c, DS_ERR_ARG, q.who, "unknown curve");
        cv.kind[k] = kinds[k], cv.level[k] = par[3 * k], cv.offset[k] = par[3 * k + 1], cv.mix[k] = par[3 * k + 2];
    }
    const size_t n_st = (size_t)n_str * dsfx::STAT, n_pk = (size_t)n_str * dsfx::MAX_CURVES;
    return fx_io(c, q, n_st + n_pk, [&](auto src, auto dst) {
        using T = typename decltype(src)::type;
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, n_st}, {8, n_pk}}, t));
        const dsfx::ShapeArgs<T> a{src, dst, n, cv, gain, (const double*)t[0], (double*)t[1]};
        CHK(fx_stats(c, src, n, n_str, 1.0, (double*)t[0]));
        CHK(launch(c, "fx_curve_peak", dsfx::k_fx_curve_peak<T>, dim3((unsigned)n_str, (unsigned)n_curves), dsfx::NT, 0, a));
        return launch(c, "fx_shape", dsfx::k_fx_shape<T>, fx_grid(n, n_str), dsfx::NT, 0, a);
    });
}

// mod: host [n], the modulator every stream is multiplied by
extern "C" int ds_fx_tremolo(ds_ctx* c, const void* x, int on_device, int n_str, int64_t ldx, int64_t n, const double* mod,
                             void* y, int64_t ld_y) {
    const FxCall q{"ds_fx_tremolo", x, on_device, n_str, ldx, n, n, y, ld_y};
    CHK(fx_check(c, q));
    if (!mod) return fail(c, DS_ERR_ARG, q.who, "null argument");
    return fx_io(c, q, (size_t)n, [&](auto src, auto dst) {
        using T = typename decltype(src)::type;
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, (size_t)n, mod}}, t));
        return launch(c, "fx_tremolo", dsfx::k_fx_tremolo<T>, fx_grid(n, n_str), dsfx::NT, 0,
                      dsfx::TremoloArgs<T>{src, dst, n, (const double*)t[0]});
    });
}

// ---- spectral subtraction (kernels_specsub.hpp), float64 --------------------------------------------------------------
// win_a, win_s: host [W], the analysis and the synthesis window; table: host [n_str][W / 2 + 1], |noise PSD|^(e / 2) of
// every stream (DS_FX_SPECSUB_STATIC; not read otherwise); env_floor: the envelope's floor, negative for none.
extern "C" int ds_fx_specsub(ds_ctx* c, const void* x, int on_device, int n_str, int64_t ldx, int64_t n, const double* win_a,
                             const double* win_s, int W, int step, int mode, double threshold_db, double forgetting,
                             double factor, double exponent, const double* table, double env_floor, void* y, int64_t ld_y) {
    const FxCall q{"ds_fx_specsub", x, on_device, n_str, ldx, n, n, y, ld_y};
    const bool is_static = mode == dsss::MODE_STATIC;
    // shape and bounds before the context is looked at: nothing here touches the device
    if (!x || !y || !win_a || !win_s || (is_static && !table)) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (n_str < 1 || n < 1 || (on_device && (ldx < n || ld_y < n))) return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (W < kSpecsubMinWindow || (W & (W - 1)) || step < 1 || step > W || (mode != dsss::MODE_ADAPTIVE && !is_static) ||
        !(forgetting > 0.0 && forgetting <= 1.0) || !(factor > 0.0) || !(exponent > 0.0))
        return fail(c, DS_ERR_ARG, q.who,
                    "needs a power-of-two window >= 4, 1 <= step <= window, a known mode, 0 < forgetting <= 1, factor > 0, exponent > 0");
    if (specsub_window_unsupported(W)) return fail(c, DS_ERR_UNSUP, q.who, "windows above 16384 samples are not built");
    if (specsub_work_too_large(n_str, n, W, step))
        return fail(c, DS_ERR_UNSUP, q.who, "a frame workspace above 2^32 bytes or more than 2^29 overlap-add terms are not built");
    CHK(fx_check(c, q));
    int lg = 0;
    while ((1 << lg) < W) ++lg;
    const dsss::Frames fr{W, lg, step, (int)specsub_frames(n, W, step), n};
    const size_t n_st = (size_t)n_str * dsfx::STAT, n_slot = (size_t)n_str * fr.n_frames * fr.pitch();
    const size_t n_gate = (size_t)n_str * fr.n_frames, n_tab = is_static ? (size_t)n_str * fr.bins() : 0;
    const size_t n_block = (size_t)((n + dsss::OLA_TILE - 1) / dsss::OLA_TILE);
    const int power = exponent == 1.0 ? dsss::POWER_ONE : (exponent == 2.0 ? dsss::POWER_TWO : dsss::POWER_ANY);
    return fx_io(c, q, 2 * n_st + q.elements() + n_slot + n_gate / 8 + 1 + 3 * (size_t)W + n_tab + n_gate + n_str * n_block + 11 * 32, [&](auto src, auto dst) {
        using T = typename decltype(src)::type;
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, n_st}, {8, n_st}, {8, q.elements()}, {8, n_slot}, {1, n_gate}, {8, (size_t)W, win_a},
                                            {8, (size_t)W, win_s}, {16, (size_t)W / 2}, {8, n_tab, table}, {8, n_gate},
                                            {8, (size_t)n_str * n_block}}, t));
        double *st_in = (double*)t[0], *st_out = (double*)t[1], *yd = (double*)t[2];
        double2 *spec = (double2*)t[3], *tw = (double2*)t[7];
        hipLaunchKernelGGL(f64c::k_twiddles, dim3((W / 2 + 255) / 256), dim3(256), 0, c->stream, tw, W / 2);
        HIPCHK(c, hipGetLastError());
        double *frame_peak = (double*)t[9], *block_peak = (double*)t[10];
        const dim3 per_frame((unsigned)fr.n_frames, (unsigned)n_str);
        CHK(launch(c, "ss_analyze", dsss::k_ss_analyze<T>, per_frame, dsss::NT, dsss::frame_lds(W),
                   dsss::AnalyzeArgs<T>{src, fr, (const double*)t[5], tw, threshold_db, spec, (uint8_t*)t[4], frame_peak}));
        const dsss::TrackArgs ta{spec, (const uint8_t*)t[4], (const double*)t[8], fr.bins(), fr.n_frames, mode, forgetting, factor, exponent};
        const dim3 tg((unsigned)dsss::track_bin_blocks(fr.bins()) * (unsigned)dsss::track_frame_tiles(fr.n_frames, mode), (unsigned)n_str);
        if (power == dsss::POWER_ONE) CHK(launch(c, "ss_track@one", dsss::k_ss_track<dsss::POWER_ONE>, tg, dsss::NT, 0, ta));
        if (power == dsss::POWER_TWO) CHK(launch(c, "ss_track@two", dsss::k_ss_track<dsss::POWER_TWO>, tg, dsss::NT, 0, ta));
        if (power == dsss::POWER_ANY) CHK(launch(c, "ss_track@pow", dsss::k_ss_track<dsss::POWER_ANY>, tg, dsss::NT, 0, ta));
        CHK(launch(c, "ss_synth", dsss::k_ss_synth, per_frame, dsss::NT, dsss::frame_lds(W),
                   dsss::SynthArgs{spec, fr, (const double*)t[6], tw}));
        CHK(launch(c, "ss_ola", dsss::k_ss_ola, dim3((unsigned)n_block, (unsigned)n_str), dsss::OLA_TILE, 0,
                   dsss::OlaArgs{(const double*)spec, fr, (const double*)t[6], env_floor, yd, block_peak}));
        CHK(launch(c, "ss_peak", dsss::k_ss_peak, dim3((unsigned)n_str, 2), dsss::NT, 0,
                   dsss::PeakArgs{frame_peak, block_peak, fr.n_frames, (int)n_block, st_in, st_out}));
        return launch(c, "fx_scale", dsfx::k_fx_scale<T>, fx_grid(n, n_str), dsfx::NT, 0,
                      dsfx::ScaleArgs<T>{yd, dst, n, dsfx::RESTORE_PEAK, st_in, st_out, 1.0});
    });
}

// ---- levels and loudness (kernels_level.hpp), float64 ---------------------------------------------------------------
// What every entry takes: x, n samples of n_ch channels, on the host as (samples, channels) float64 or on the device as
// planar float32 rows of pitch ldx.  basis: the host's [2 + 2 * 8] doubles (N - 1) / 2, 1 / sqrt(N), a_0 .. a_7,
// b_0 .. b_7 of the orthonormal recurrence (kernels_level.hpp), read up to `order`.
struct LevelCall {
    const char* who;
    const void* x;
    int on_device, n_ch;
    int64_t ldx, n;
    int n_wg() const { return (int)((n + dslevel::SPAN - 1) / dslevel::SPAN); }
    size_t elements() const { return (size_t)n_ch * (size_t)n; }
    size_t x_count() const { return on_device ? 0 : elements(); }  // what a host call stages
};

static int level_check(ds_ctx* c, const LevelCall& q, const void* out) {
    if (!c || !q.x || !out) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (q.n_ch < 1 || q.n < 1 || (q.on_device && q.ldx < q.n)) return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (level_shape_unsupported(q.n_ch, q.n))
        return fail(c, DS_ERR_UNSUP, q.who, "more than 65535 channels, 2^31 - 1 samples a channel or 2^33 samples in all are not built");
    return DS_OK;
}

// order -1: no polynomial (basis may be null)
static int level_basis(ds_ctx* c, const LevelCall& q, int order, const double* basis, dslevel::Basis* bs) {
    *bs = dslevel::Basis{};
    bs->order = order;
    if (order < 0) return DS_OK;
    if (!basis) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (order > dslevel::MAX_ORDER || order >= q.n)
        return fail(c, DS_ERR_ARG, q.who, "the polynomial order is at most 8 and below the sample count");
    bs->half = basis[0], bs->p0 = basis[1];
    for (int k = 0; k < dslevel::MAX_ORDER; ++k) {
        bs->a[k] = k < order ? basis[2 + k] : 0.0;
        bs->b[k] = k < order ? basis[2 + dslevel::MAX_ORDER + k] : 0.0;
        if (!std::isfinite(bs->a[k]) || !std::isfinite(bs->b[k])) return fail(c, DS_ERR_ARG, q.who, "the basis must be finite");
    }
    return DS_OK;
}

// run(src) over the samples where they lie; d0: the device address of a host call's staged samples
template <class F>
static int level_src(const LevelCall& q, const void* d0, F&& run) {
    if (q.on_device) return run(dslevel::Src<float>{(const float*)q.x, 1, q.ldx});
    return run(dslevel::Src<double>{(const double*)d0, q.n_ch, 1});
}

// c_0 .. c_order and max |x| of every channel: partial [n_ch][n_wg][NC] -> out_dev [n_ch][NC]
template <typename T>
static int level_project(ds_ctx* c, const LevelCall& q, dslevel::Src<T> x, const dslevel::Basis& bs, double* partial,
                         double* out_dev) {
    CHK(launch(c, "level_project", dslevel::k_level_project<T>, dim3((unsigned)q.n_wg(), (unsigned)q.n_ch), dslevel::NT, 0,
               dslevel::ProjectArgs<T>{x, q.n, q.n_wg(), bs, partial}));
    return launch(c, "level_final@project", dslevel::k_level_final<dslevel::MAX_ORDER + 1, 1>, dim3((unsigned)q.n_ch), dslevel::NT, 0,
                  dslevel::FinalArgs{partial, q.n_wg(), out_dev});
}

// sum r^2, max |r|, max |x| of r = x - p(n): partial [n_ch][n_wg][NST] -> out_dev [n_ch][NST]
template <typename T>
static int level_stats(ds_ctx* c, const LevelCall& q, dslevel::Src<T> x, const dslevel::Basis& bs, const double* coef,
                       double* partial, double* out_dev) {
    CHK(launch(c, "level_stats", dslevel::k_level_stats<T>, dim3((unsigned)q.n_wg(), (unsigned)q.n_ch), dslevel::NT, 0,
               dslevel::StatsArgs<T>{x, q.n, q.n_wg(), bs, coef, partial}));
    return launch(c, "level_final@stats", dslevel::k_level_final<1, 2>, dim3((unsigned)q.n_ch), dslevel::NT, 0,
                  dslevel::FinalArgs{partial, q.n_wg(), out_dev});
}

static size_t level_partial_count(const LevelCall& q) { return (size_t)q.n_ch * q.n_wg() * dslevel::NC; }

// out: host (n_ch, 10): c_0 .. c_8 (zero past the order), max |x|
extern "C" int ds_level_project(ds_ctx* c, const void* x, int on_device, int n_ch, int64_t ldx, int64_t n, int order,
                                const double* basis, double* out) {
    const LevelCall q{"ds_level_project", x, on_device, n_ch, ldx, n};
    CHK(level_check(c, q, out));
    dslevel::Basis bs;
    if (order < 0) return fail(c, DS_ERR_ARG, q.who, "needs an order >= 0");
    CHK(level_basis(c, q, order, basis, &bs));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_rec = (size_t)n_ch * dslevel::NC;
    CHK(mem_check(c, q.who, level_partial_count(q) * 8, (q.x_count() + n_rec) * 8, 0));
    return staged(c, {{8, q.x_count(), x}, {8, n_rec, nullptr, out}}, [&](void* const* d) {
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, level_partial_count(q)}}, t));
        return level_src(q, d[0], [&](auto src) { return level_project(c, q, src, bs, (double*)t[0], (double*)d[1]); });
    });
}

// out: host (n_ch, 3): sum (x - p)^2, max |x - p|, max |x|, p the least-squares polynomial of `order` of each channel;
// with `common` (order 0 only) the mean of all channels together
extern "C" int ds_level_stats(ds_ctx* c, const void* x, int on_device, int n_ch, int64_t ldx, int64_t n, int order,
                              const double* basis, int common, double* out) {
    const LevelCall q{"ds_level_stats", x, on_device, n_ch, ldx, n};
    CHK(level_check(c, q, out));
    dslevel::Basis bs;
    if (order < 0 || (common && order != 0)) return fail(c, DS_ERR_ARG, q.who, "needs an order >= 0, and 0 with a common mean");
    CHK(level_basis(c, q, order, basis, &bs));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_rec = (size_t)n_ch * dslevel::NC, n_st = (size_t)n_ch * dslevel::NST;
    CHK(mem_check(c, q.who, (level_partial_count(q) + n_rec) * 8 + 256, (q.x_count() + n_st) * 8, 0));
    return staged(c, {{8, q.x_count(), x}, {8, n_st, nullptr, out}}, [&](void* const* d) {
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, level_partial_count(q)}, {8, n_rec}}, t));
        double *partial = (double*)t[0], *coef = (double*)t[1];
        return level_src(q, d[0], [&](auto src) {
            CHK(level_project(c, q, src, bs, partial, coef));
            if (common) CHK(launch(c, "level_common", dslevel::k_level_common, dim3(1), 64, 0, dslevel::CommonArgs{coef, n_ch}));
            return level_stats(c, q, src, bs, coef, partial, (double*)d[1]);
        });
    });
}

// y[n] = (x[n] - p_c(n)) g_c fade[n] fade[N - 1 - n]; y as x: host (n, n_ch) float64 or planar float32 rows of pitch ld_y
extern "C" int ds_level_apply(ds_ctx* c, const void* x, int on_device, int n_ch, int64_t ldx, int64_t n, int order,
                              const double* basis, int norm_mode, double norm_factor, const double* gain, const double* fade,
                              int64_t l_fade, int at_start, int at_end, void* y, int64_t ld_y) {
    const LevelCall q{"ds_level_apply", x, on_device, n_ch, ldx, n};
    CHK(level_check(c, q, y));
    if (on_device && ld_y < n) return fail(c, DS_ERR_ARG, q.who, "bad shape");
    if (norm_mode < dslevel::NORM_NONE || norm_mode > dslevel::NORM_RMS_ALL || (norm_mode != dslevel::NORM_NONE && gain))
        return fail(c, DS_ERR_ARG, q.who, "needs a known normalisation, and no gains beside one");
    if (fade && (l_fade < 1 || l_fade > n || !(at_start || at_end)))
        return fail(c, DS_ERR_ARG, q.who, "a fade has 1 .. n samples and an end to apply to");
    dslevel::Basis bs, bs0;
    CHK(level_basis(c, q, order, basis, &bs));
    const bool norm = norm_mode != dslevel::NORM_NONE, rms = norm_mode >= dslevel::NORM_RMS_EACH;
    const double mean_basis[2 + 2 * dslevel::MAX_ORDER] = {0.5 * (double)(n - 1), 1.0 / std::sqrt((double)n)};
    CHK(level_basis(c, q, norm ? 0 : -1, mean_basis, &bs0));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_rec = (size_t)n_ch * dslevel::NC, n_st = (size_t)n_ch * dslevel::NST, n_fade = fade ? (size_t)l_fade : 0;
    const size_t n_io = on_device ? 0 : q.elements();
    CHK(mem_check(c, q.who, (level_partial_count(q) + 2 * n_rec + n_st + n_ch + n_fade) * 8 + 6 * 256, 2 * n_io * 8, 0));
    return staged(c, {{8, n_io, x}, {8, n_io, nullptr, on_device ? nullptr : y}}, [&](void* const* d) {
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, level_partial_count(q)}, {8, n_rec}, {8, n_rec}, {8, n_st}, {8, (size_t)n_ch, gain},
                                            {8, n_fade, fade}}, t));
        double *partial = (double*)t[0], *coef = (double*)t[1], *proj0 = (double*)t[2], *stats = (double*)t[3], *g = (double*)t[4];
        const dslevel::ApplyArgs a{n, n_ch, bs, coef, gain || norm ? g : nullptr, fade ? (const double*)t[5] : nullptr, l_fade,
                                   at_start, at_end};
        CHK(level_src(q, d[0], [&](auto src) {
            if (order >= 0) CHK(level_project(c, q, src, bs, partial, coef));
            if (norm) {
                CHK(level_project(c, q, src, bs0, partial, proj0));
                if (norm_mode == dslevel::NORM_RMS_ALL)
                    CHK(launch(c, "level_common", dslevel::k_level_common, dim3(1), 64, 0, dslevel::CommonArgs{proj0, n_ch}));
                if (rms) CHK(level_stats(c, q, src, bs0, proj0, partial, stats));
                CHK(launch(c, "level_gain", dslevel::k_level_gain, dim3(1), 64, 0,
                           dslevel::GainArgs{norm_mode, n_ch, n, norm_factor, proj0, stats, g}));
            }
            return DS_OK;
        }));
        if (on_device)
            return launch(c, "level_apply@f4", dslevel::k_level_apply_f4, dim3((unsigned)((n / 4 + 2 + dslevel::NT - 1) / dslevel::NT), (unsigned)n_ch),
                          dslevel::NT, 0, dslevel::ApplyF4{(const float*)x, ldx, (float*)y, ld_y, a});
        const int64_t pairs = ((int64_t)q.elements() + 1) / 2;
        return launch(c, "level_apply@d2", dslevel::k_level_apply_d2, dim3((unsigned)((pairs + dslevel::NT - 1) / dslevel::NT)), dslevel::NT, 0,
                      dslevel::ApplyD2{(const double*)d[0], (double*)d[1], a});
    });
}

// out: host (n, n_ch) float64: sqrt(max(0, mean of the last w squares of x - line)), zeros before the first sample
extern "C" int ds_moving_rms(ds_ctx* c, const void* x, int on_device, int n_ch, int64_t ldx, int64_t n, const double* basis,
                             int64_t w, double* out) {
    const LevelCall q{"ds_moving_rms", x, on_device, n_ch, ldx, n};
    CHK(level_check(c, q, out));
    if (w < 1) return fail(c, DS_ERR_ARG, q.who, "needs a window of at least one sample");
    if (level_moving_work_too_large(n_ch, n, w)) return fail(c, DS_ERR_UNSUP, q.who, "a window this long on a signal this long is not built");
    dslevel::Basis bs;
    CHK(level_basis(c, q, n > 1 ? 1 : 0, basis, &bs));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_rec = (size_t)n_ch * dslevel::NC;
    CHK(mem_check(c, q.who, (level_partial_count(q) + n_rec) * 8 + 256, (q.x_count() + q.elements()) * 8, 0));
    return staged(c, {{8, q.x_count(), x}, {8, q.elements(), nullptr, out}}, [&](void* const* d) {
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, level_partial_count(q)}, {8, n_rec}}, t));
        double *partial = (double*)t[0], *coef = (double*)t[1];
        return level_src(q, d[0], [&](auto src) {
            using T = typename decltype(src)::type;
            CHK(level_project(c, q, src, bs, partial, coef));
            return launch(c, "level_moving", dslevel::k_level_moving<T>, dim3((unsigned)((n + dslevel::TILE - 1) / dslevel::TILE), (unsigned)n_ch),
                          dslevel::NT, 0, dslevel::MovingArgs<T>{src, n, w, n_ch, bs, coef, (double*)d[1]});
        });
    });
}

// sos: host [n_sec][6], the weighting cascade; z: host (n_blocks, n_ch) float64, block b the mean square of the weighted
// samples b step .. b step + tg - 1; n_blocks must be ceil((n - tg) / step) >= 1
extern "C" int ds_loudness_blocks(ds_ctx* c, const void* x, int on_device, int n_ch, int64_t ldx, int64_t n, const double* sos,
                                  int n_sec, int64_t tg, int64_t step, int64_t n_blocks, double* z) {
    const LevelCall q{"ds_loudness_blocks", x, on_device, n_ch, ldx, n};
    CHK(level_check(c, q, z));
    if (!sos) return fail(c, DS_ERR_ARG, q.who, "null argument");
    if (n_sec < 1) return fail(c, DS_ERR_ARG, q.who, "needs at least one section");
    if (n_sec > iir::MAX_SEC) return fail(c, DS_ERR_UNSUP, q.who, "more than 32 second-order sections in one cascade is not built");
    for (int i = 0; i < 6 * n_sec; ++i)
        if (!std::isfinite(sos[i]) || (i % 6 == 3 && sos[i] == 0.0))
            return fail(c, DS_ERR_ARG, q.who, "sections must be finite with a0 != 0");
    if (tg < 1 || step < 1 || n <= tg || n_blocks != (n - tg + step - 1) / step)
        return fail(c, DS_ERR_ARG, q.who, "needs more samples than one block, and ceil((n - tg) / step) blocks");
    if (n_blocks > INT32_MAX) return fail(c, DS_ERR_UNSUP, q.who, "more than 2^31 - 1 blocks are not built");
    const IirCall iq{q.who, n_ch, n, n, n, sos, 1, n_sec, DS_FB_PARALLEL};
    HIPCHK(c, hipSetDevice(c->device));
    // the float64 planar copy of resident samples and the weighted samples are pieces of c->io: the sos runner carves c->ws
    const size_t n_wide = on_device ? q.elements() : 0, n_z = (size_t)n_blocks * n_ch;
    const size_t n_groups = (size_t)((n + carry::G - 1) / carry::G);
    CHK(mem_check(c, q.who, ((size_t)n_ch * n_groups * 2 * n_sec + 64 * (size_t)n_sec * n_sec) * 8 + 4 * 256,
                  (q.x_count() + n_wide + q.elements() + n_z) * 8, 0));
    return staged(c, {{8, q.x_count(), x}, {8, n_wide}, {8, q.elements()}, {8, n_z, nullptr, z}}, [&](void* const* d) {
        double *wide = (double*)d[1], *yd = (double*)d[2];
        if (on_device) {
            dslevel::ApplyArgs a{};
            a.n = n, a.n_ch = n_ch, a.bs.order = -1;
            CHK(launch(c, "level_apply@widen", dslevel::k_level_apply<float, double>, dim3((unsigned)((n + dslevel::NT - 1) / dslevel::NT), (unsigned)n_ch),
                       dslevel::NT, 0, dslevel::ApplyAny<float, double>{dslevel::Src<float>{(const float*)x, 1, ldx}, dslevel::Dst<double>{wide, 1, n}, a}));
            CHK(iir_run<double>(c, iq, wide, n, 1, nullptr, yd, (int64_t)q.elements(), n, 1, nullptr));
        } else {
            CHK(iir_run<double>(c, iq, (const double*)d[0], 1, n_ch, nullptr, yd, (int64_t)q.elements(), n, 1, nullptr));
        }
        return launch(c, "level_blocks", dslevel::k_level_blocks, dim3((unsigned)n_blocks, (unsigned)n_ch), dslevel::NT, 0,
                      dslevel::BlockArgs{yd, n, tg, step, n_ch, (double*)d[3]});
    });
}

// out: host (n, n_ch) float64: |analytic signal| of x minus its least-squares line
extern "C" int ds_envelope_analytic(ds_ctx* c, const void* x, int on_device, int n_ch, int64_t ldx, int64_t n, const double* basis,
                                    double* out) {
    const LevelCall q{"ds_envelope_analytic", x, on_device, n_ch, ldx, n};
    CHK(level_check(c, q, out));
    dslevel::Basis bs;
    CHK(level_basis(c, q, n > 1 ? 1 : 0, basis, &bs));
    const size_t n_rec = (size_t)n_ch * dslevel::NC;
    Fft64Run r{c, {}, n_ch};
    CHK(fft64_plan(c, q.who, n, n_ch, level_partial_count(q) * 8 + 256, (q.x_count() + 2 * q.elements() + n_rec) * 8 + 4 * 256, &r.pl));
    // the detrended samples and the coefficients are pieces of c->io: the transform carves c->ws
    return staged(c, {{8, q.x_count(), x}, {8, q.elements()}, {8, n_rec}, {8, q.elements(), nullptr, out}}, [&](void* const* d) {
        void* t[kMaxStaged];
        CHK(stage(c, &c->ws, &c->ws_bytes, {{8, level_partial_count(q)}}, t));
        double *det = (double*)d[1], *coef = (double*)d[2];
        const dslevel::ApplyArgs a{n, n_ch, bs, coef, nullptr, nullptr, 0, 0, 0};
        CHK(level_src(q, d[0], [&](auto src) {
            using T = typename decltype(src)::type;
            CHK(level_project(c, q, src, bs, (double*)t[0], coef));
            return launch(c, "level_apply@detrend", dslevel::k_level_apply<T, double>, dim3((unsigned)((n + dslevel::NT - 1) / dslevel::NT), (unsigned)n_ch),
                          dslevel::NT, 0, dslevel::ApplyAny<T, double>{src, dslevel::Dst<double>{det, n_ch, 1}, a});
        }));
        CHK(r.carve_ws(0));
        CHK(r.load(det, false, n));
        CHK(r.fft(false));
        CHK(r.point(fft64::POINT_MASK, 1.0));
        CHK(r.fft(true));
        return launch(c, "level_mag", dslevel::k_level_mag, dim3((unsigned)((q.elements() + dslevel::NT - 1) / dslevel::NT)), dslevel::NT, 0,
                      dslevel::MagArgs{r.x, r.pl.ld, n, n_ch, 1.0 / (double)n, (double*)d[3]});
    });
}

// ---- RCCL (resolved at run time so the library loads on machines without it) ----
typedef int (*nccl_getuid_t)(void*);
struct uid128 {
    char b[128];
};
typedef int (*nccl_init_rank_t)(void**, int, uid128, int);
typedef int (*nccl_bcast_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_allgather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*nccl_destroy_t)(void*);
typedef const char* (*nccl_errstr_t)(int);

static void* rccl_handle() {
    static void* h = nullptr;
    // reuse a copy the host process already mapped (e.g. the one PyTorch links) before loading one
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW);
    if (!h) h = dlopen("librccl.so", RTLD_NOW);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW);
    return h;
}

extern "C" int ds_comm_unique_id(char id_out[128]) {
    if (!id_out) return fail(nullptr, DS_ERR_ARG, "ds_comm_unique_id: null");
    void* h = rccl_handle();
    if (!h) return fail(nullptr, DS_ERR_COMM, "librccl.so not found");
    auto f = (nccl_getuid_t)dlsym(h, "ncclGetUniqueId");
    if (!f) return fail(nullptr, DS_ERR_COMM, "ncclGetUniqueId missing");
    int r = f(id_out);
    return r == 0 ? DS_OK : fail(nullptr, DS_ERR_COMM, "ncclGetUniqueId failed");
}

extern "C" int ds_comm_init(ds_ctx* c, int n_ranks, int rank, const char id[128]) {
    if (!c || !id || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return fail(c, DS_ERR_ARG, "ds_comm_init: bad argument");
    void* h = rccl_handle();
    if (!h) return fail(c, DS_ERR_COMM, "librccl.so not found");
    auto f = (nccl_init_rank_t)dlsym(h, "ncclCommInitRank");
    if (!f) return fail(c, DS_ERR_COMM, "ncclCommInitRank missing");
    HIPCHK(c, hipSetDevice(c->device));
    uid128 u;
    memcpy(u.b, id, 128);
    int r = f(&c->comm, n_ranks, u, rank);
    if (r != 0) {
        auto es = (nccl_errstr_t)dlsym(h, "ncclGetErrorString");
        return fail(c, DS_ERR_COMM, std::string("ncclCommInitRank: ") + (es ? es(r) : "error"));
    }
    c->rccl = h;
    return DS_OK;
}

// ranks of the library's communicator as RCCL itself counts them (ncclCommCount)
extern "C" int ds_comm_count(ds_ctx* c, int* n_ranks) {
    if (!c || !n_ranks) return fail(c, DS_ERR_ARG, "ds_comm_count: null argument");
    if (!c->comm) return fail(c, DS_ERR_COMM, "ds_comm_count: communicator not initialised");
    typedef int (*nccl_count_t)(void*, int*);
    auto f = (nccl_count_t)dlsym(c->rccl, "ncclCommCount");
    if (!f) return fail(c, DS_ERR_COMM, "ncclCommCount missing");
    if (f(c->comm, n_ranks) != 0) return fail(c, DS_ERR_COMM, "ncclCommCount failed");
    return DS_OK;
}

extern "C" int ds_bcast(ds_ctx* c, void* buf, size_t bytes, int root) {
    if (!c || !buf) return fail(c, DS_ERR_ARG, "ds_bcast: null argument");
    if (!c->comm) return fail(c, DS_ERR_COMM, "ds_bcast: communicator not initialised");
    auto f = (nccl_bcast_t)dlsym(c->rccl, "ncclBroadcast");
    if (!f) return fail(c, DS_ERR_COMM, "ncclBroadcast missing");
    int r = f(buf, buf, bytes, /*ncclChar*/ 0, root, c->comm, c->stream);
    if (r != 0) return fail(c, DS_ERR_COMM, "ncclBroadcast failed");
    return DS_OK;
}

extern "C" int ds_allgather(ds_ctx* c, const void* send, void* recv, size_t bytes_per_rank) {
    if (!c || !send || !recv) return fail(c, DS_ERR_ARG, "ds_allgather: null argument");
    if (!c->comm) return fail(c, DS_ERR_COMM, "ds_allgather: communicator not initialised");
    auto f = (nccl_allgather_t)dlsym(c->rccl, "ncclAllGather");
    if (!f) return fail(c, DS_ERR_COMM, "ncclAllGather missing");
    int r = f(send, recv, bytes_per_rank, /*ncclChar*/ 0, c->comm, c->stream);
    if (r != 0) return fail(c, DS_ERR_COMM, "ncclAllGather failed");
    return DS_OK;
}

// ---- measured copy bandwidth (the roofline's second denominator) --------------
__global__ __launch_bounds__(256) void k_copy16(const float4* __restrict__ src, float4* __restrict__ dst, size_t n16) {
    // four independent 16-byte loads per lane in flight before the first store
    const size_t stride = (size_t)gridDim.x * 1024;
    size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x;
    for (; i + 768 < n16; i += stride) {
        const float4 a = src[i], b = src[i + 256], c = src[i + 512], d = src[i + 768];
        dst[i] = a;
        dst[i + 256] = b;
        dst[i + 512] = c;
        dst[i + 768] = d;
    }
    if (i < n16) {  // the last, partly filled tile
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + 256 * k < n16) dst[i + 256 * k] = src[i + 256 * k];
    }
}
extern "C" int ds_measure_copy(ds_ctx* c, size_t bytes, int reps, double* gb_per_s) {
    if (!c || !gb_per_s || bytes < 16 || reps <= 0) return fail(c, DS_ERR_ARG, "ds_measure_copy: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    float4 *a = nullptr, *b = nullptr;
    const size_t n16 = bytes / 16;
    if (hipMalloc((void**)&a, n16 * 16) != hipSuccess) return fail(c, DS_ERR_NOMEM, "ds_measure_copy: hipMalloc");
    if (hipMalloc((void**)&b, n16 * 16) != hipSuccess) {
        (void)hipFree(a);
        return fail(c, DS_ERR_NOMEM, "ds_measure_copy: hipMalloc");
    }
    int rc = DS_OK;
    float ms = 0.f;
    const unsigned grid = (unsigned)std::min<size_t>((n16 + 1023) / 1024, 256 * 8);  // 8 workgroups per CU
    do {
        if (hipMemsetAsync(a, 1, n16 * 16, c->stream) != hipSuccess) { rc = fail(c, DS_ERR_HIP, "ds_measure_copy: memset"); break; }
        hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(256), 0, c->stream, a, b, n16);
        if (hipEventRecord(c->ev0, c->stream) != hipSuccess) { rc = fail(c, DS_ERR_HIP, "ds_measure_copy: event"); break; }
        for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(256), 0, c->stream, a, b, n16);
        if (hipEventRecord(c->ev1, c->stream) != hipSuccess || hipEventSynchronize(c->ev1) != hipSuccess ||
            hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess || hipGetLastError() != hipSuccess) {
            rc = fail(c, DS_ERR_HIP, "ds_measure_copy: timing");
            break;
        }
        *gb_per_s = 2.0 * (double)(n16 * 16) * reps / ((double)ms * 1e-3) / 1e9;
    } while (0);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(a);
    (void)hipFree(b);
    return rc;
}

extern "C" int ds_mem_info(ds_ctx* c, size_t* free_bytes, size_t* total_bytes) {
    if (!c || !free_bytes || !total_bytes) return fail(c, DS_ERR_ARG, "ds_mem_info: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemGetInfo(free_bytes, total_bytes));
    return DS_OK;
}

extern "C" int ds_comm_destroy(ds_ctx* c) {
    if (!c || !c->comm) return DS_OK;
    auto f = (nccl_destroy_t)dlsym(c->rccl, "ncclCommDestroy");
    if (f) f(c->comm);
    c->comm = nullptr;
    return DS_OK;
}
