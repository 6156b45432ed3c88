// capi.hip -- library-level entry points: error strings, version, hardware probe.
#include <atomic>
#include <mutex>
#include <stdlib.h>
#include <vector>
#include "common.hpp"

extern "C" const char* morec_strerror(int code) {
    switch (code) {
        case MOREC_OK: return "ok";
        case MOREC_E_ARG: return "MOREC_E_ARG: null pointer or non-positive size";
        case MOREC_E_ALIGN: return "MOREC_E_ALIGN: pointer/pitch not 16-byte aligned or size not a vector multiple";
        case MOREC_E_UNSUPPORTED: return "MOREC_E_UNSUPPORTED: shape outside kernel limits";
        case MOREC_E_DTYPE: return "MOREC_E_DTYPE: unsupported dtype combination";
        case MOREC_E_COMM: return "MOREC_E_COMM: an RCCL call failed (morec_comm_last_error)";
        default: break;
    }
    if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
    return "unknown morec error";
}

extern "C" int morec_version(void) { return 105; }

// Process-wide dropout seed source (see morec_hip.h): a device uint64 folded into every dropout / DropPath stream at kernel entry.
static const uint64_t* g_drop_seed_src = nullptr;
const uint64_t* morec_drop_seed_src() { return g_drop_seed_src; }
extern "C" int morec_dropout_seed_source(const void* dev_u64) {
    if (reinterpret_cast<uintptr_t>(dev_u64) & 7u) return MOREC_E_ALIGN;
    g_drop_seed_src = reinterpret_cast<const uint64_t*>(dev_u64);
    return MOREC_OK;
}

// ---- deterministic mode (common.hpp; the switch itself is a row of the knob table, tuning.hip) ---------------------------------------
// Library-owned partial-sum scratch of the deterministic mode, one buffer per (device, stream) -- launches on a stream are ordered, so they
// share it.  nullptr = "not available": the callers return an error (never a silent fall-back to the atomic kernels).  Growth frees and
// reallocates, which a stream that is being CAPTURED must not do (a graph would keep the freed address): under capture a request the
// buffer cannot hold is refused -- run the shapes once eagerly (TrainStep does: its warm-up steps precede capture) or call
// morec_det_scratch_reserve.  Sixteen (device, stream) pairs; beyond that the least recently used buffer is dropped behind a device sync.
// While a deferred-fold scope is open on `s` (below) the request is served by that scope's bump allocator instead: every producer gets a
// region of its own that stays intact until the flush that reads it has run.
float* morec_det_scratch(hipStream_t s, size_t n) {
    if (morec_fold_deferring(s)) return morec_fold_scratch(s, n);
    struct Slot { hipStream_t s; int dev; float* p; size_t n; unsigned long long used; };
    static Slot slots[16];
    static int n_slots = 0;
    static unsigned long long tick = 0;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    const bool capturing = cap != hipStreamCaptureStatusNone;
    Slot* sl = nullptr;
    for (int i = 0; i < n_slots; ++i)
        if (slots[i].s == s && slots[i].dev == dev) sl = &slots[i];
    if (!sl) {
        if (capturing) return nullptr;
        if (n_slots < 16) {
            sl = &slots[n_slots++];
        } else {      // evict the least recently used pair of THIS device (its stream may be gone: wait for the device, not for the stream)
            for (int i = 0; i < n_slots; ++i)
                if (slots[i].dev == dev && (!sl || slots[i].used < sl->used)) sl = &slots[i];
            if (!sl) return nullptr;
            (void)hipDeviceSynchronize();
            if (sl->p) (void)hipFree(sl->p);
        }
        *sl = Slot{s, dev, nullptr, 0, 0};
    }
    sl->used = ++tick;
    if (sl->n < n) {
        if (capturing) return nullptr;
        if (sl->p) {      // launches that still read the old buffer are on this stream
            (void)hipStreamSynchronize(s);
            (void)hipFree(sl->p);
            sl->p = nullptr; sl->n = 0;
        }
        size_t want = n + n / 4;
        if (want < ((size_t)1 << 20)) want = (size_t)1 << 20;
        if (hipMalloc(reinterpret_cast<void**>(&sl->p), want * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); sl->p = nullptr; return nullptr; }
        sl->n = want;
    }
    return sl->p;
}
// Pre-size the deterministic mode's scratch of `stream` to `n_floats` (outside graph capture): see include/morec_hip.h.
extern "C" int morec_det_scratch_reserve(size_t n_floats, void* stream) {
    return morec_det_scratch(reinterpret_cast<hipStream_t>(stream), n_floats) ? MOREC_OK : (int)hipErrorOutOfMemory;
}

// 16 columns x 16 partial groups per block: group g sums the partials g, g + 16, ... in four chains, then thread g == 0 of each column adds
// the 16 group sums in group order -- a fixed summation order, and 16x fewer dependent loads per thread than one thread per column (a
// LayerNorm fold of ~500 partial rows took 36 us as one thread per column: profiles/det_mode_step.txt)
__global__ __launch_bounds__(256) void det_fold_add_kernel(const float* __restrict__ part, float* __restrict__ dst, int n_parts, size_t n, size_t stride) {
    __shared__ float red[16][17];
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
    const size_t j = blockIdx.x * (size_t)16 + c;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (j < n) {
        int p = g;
        for (; p + 48 < n_parts; p += 64) {
            a0 += part[(size_t)p * stride + j];
            a1 += part[(size_t)(p + 16) * stride + j];
            a2 += part[(size_t)(p + 32) * stride + j];
            a3 += part[(size_t)(p + 48) * stride + j];
        }
        for (; p < n_parts; p += 16) a0 += part[(size_t)p * stride + j];
    }
    red[g][c] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (g == 0 && j < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][c];
        dst[j] += t;
    }
}
int morec_det_fold_add(const float* part, float* dst, int n_parts, size_t n, size_t stride, hipStream_t s) {
    if (n == 0 || n_parts <= 0) return MOREC_OK;
    if (morec_fold_defer(part, dst, n, n_parts, stride, 0, s)) return MOREC_OK;      // an open scope on s: queued, launched by morec_fold_flush
    return morec_det_fold_add_now(part, dst, n_parts, n, stride, s);
}
int morec_det_fold_add_now(const float* part, float* dst, int n_parts, size_t n, size_t stride, hipStream_t s) {
    if (n == 0 || n_parts <= 0) return MOREC_OK;
    hipLaunchKernelGGL(det_fold_add_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, part, dst, n_parts, n, stride);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// ---- deferred folds (include/morec_hip.h: morec_fold_defer_begin / morec_fold_flush / morec_fold_defer_end) ------------------------------
// Every fold of the deterministic mode writes a PARAMETER gradient (a bias, a LayerNorm weight, a position row) that nothing in the
// backward pass reads, yet each launch is a link of the chain ln_bwd -> GEMM -> GEMM -> ...: ~140 tiny launches per encoder step between
// the heavy kernels.  While a scope is open on a producer stream, morec_det_fold_add and colsum_f32_launch (gemm.hip) on that stream only
// append a job to a host-side list; morec_fold_flush launches the list as ONE kernel (per 64 jobs) on whatever stream it is given -- the
// weight-gradient stream, once per gradient bucket.  The partial rows come from a bump allocator over library-owned chunks (a region is
// handed out once per scope: it stays intact until morec_fold_defer_end rewinds, which the caller places behind the point where the
// producer stream has waited for the flushing stream); column-sum jobs read a CALLER-owned buffer, which the caller keeps alive likewise.
// Chunks are added by hipMalloc while the first steps find the size and merged into one at the end of such a scope: a steady-state step
// allocates nothing.  A stream that is being captured opens no scope (its folds launch in place, as without the knob).  One scope at a
// time and one device per process (like the event ring of morec_stream_wait_stream below): the scratch lives on the device of its first use.
namespace {
constexpr int FOLD_MAX_JOBS = 64;
struct FoldJob {
    const float* src;
    float* dst;
    unsigned n;        // columns
    unsigned cnt;      // fold: partial rows; colsum: input rows
    unsigned stride;   // floats between rows of src
    unsigned rpb;      // 0: fold; otherwise colsum with this many input rows per row block
    unsigned blk0;     // first block of this job in the batch's grid
    unsigned pad_;
};
struct FoldBatch {
    int n_jobs, pad_;
    FoldJob job[FOLD_MAX_JOBS];      // 2.5 KB of kernel arguments: no staging buffer to recycle
};
struct FoldChunk { float* p; size_t n; };
struct FoldState {
    std::mutex mu;
    bool open = false;
    hipStream_t producer = nullptr;
    std::vector<FoldJob> queue;
    std::vector<FoldChunk> chunks;      // the last one is being bumped
    size_t used = 0;                    // floats handed out of chunks.back()
    unsigned long long n_alloc = 0, n_jobs = 0, n_launch = 0;
};
FoldState g_fold;
constexpr size_t FOLD_ALIGN = 64;                     // floats: regions start on 256-byte boundaries
constexpr size_t FOLD_CHUNK_MIN = (size_t)16 << 20;   // floats (64 MiB)
}  // namespace

// One wave per 4 columns, lane = (column c, group g) with the 16 groups of a column inside ONE wave: the group sums are combined with
// cross-lane reads (no LDS allocation, so a block can be placed on a CU whose LDS a resident GEMM workgroup holds entirely).
//   fold:   det_fold_add_kernel's tree -- partial p belongs to group p % 16, four chains per group, (a0 + a1) + (a2 + a3), remainder into a0,
//           the 16 group sums added in group order, dst += t;
//   colsum: colsum_kernel<float>(det = 1) -- row lane g of row block b sums rows r0 + g, r0 + g + 16, ..., the 16 lanes are added in lane
//           order -- and its row-block sums go through the same fold tree (block b in the place of partial b).
__global__ __launch_bounds__(256) void fold_batch_kernel(const FoldBatch b) {
    int ji = 0;
    while (ji + 1 < b.n_jobs && blockIdx.x >= b.job[ji + 1].blk0) ++ji;
    const float* __restrict__ src = b.job[ji].src;
    float* __restrict__ dst = b.job[ji].dst;
    const unsigned n = b.job[ji].n, rpb = b.job[ji].rpb;
    const int cnt = (int)b.job[ji].cnt;
    const size_t stride = b.job[ji].stride;
    const int lane = threadIdx.x & 63, c = lane & 3, g = lane >> 2;
    const size_t j = ((size_t)(blockIdx.x - b.job[ji].blk0) * 4 + (threadIdx.x >> 6)) * 4 + c;
    const bool live = j < n;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (rpb == 0) {
        if (live) {
            int p = g;
            for (; p + 48 < cnt; p += 64) {
                a0 += src[(size_t)p * stride + j];
                a1 += src[(size_t)(p + 16) * stride + j];
                a2 += src[(size_t)(p + 32) * stride + j];
                a3 += src[(size_t)(p + 48) * stride + j];
            }
            for (; p < cnt; p += 16) a0 += src[(size_t)p * stride + j];
        }
    } else {
        const int nb = (cnt + (int)rpb - 1) / (int)rpb;
        for (int blk = 0; blk < nb; ++blk) {
            const int r0 = blk * (int)rpb, r1 = min(cnt, r0 + (int)rpb);
            float s = 0.f;
            if (live) {
#pragma unroll 4
                for (int r = r0 + g; r < r1; r += 16) s += src[(size_t)r * stride + j];
            }
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) t += __shfl(s, k * 4 + c);
            // the place of partial `blk` in the fold tree: group blk % 16; chain (blk / 16) % 4 inside the four-chain rounds, a0 behind them
            const int gi = blk & 15;
            const int ch = ((blk & ~63) + gi + 48 < nb) ? (blk >> 4) & 3 : 0;
            if (g == gi) {
                if (ch == 0) a0 += t;
                else if (ch == 1) a1 += t;
                else if (ch == 2) a2 += t;
                else a3 += t;
            }
        }
    }
    const float v = (a0 + a1) + (a2 + a3);
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += __shfl(v, k * 4 + c);
    if (g == 0 && live) dst[j] += t;
}

bool morec_fold_deferring(hipStream_t s) {
    std::lock_guard<std::mutex> lock(g_fold.mu);
    return g_fold.open && g_fold.producer == s;
}

float* morec_fold_scratch(hipStream_t s, size_t n) {
    (void)s;
    std::lock_guard<std::mutex> lock(g_fold.mu);
    n = (n + FOLD_ALIGN - 1) & ~(FOLD_ALIGN - 1);
    if (g_fold.chunks.empty() || g_fold.used + n > g_fold.chunks.back().n) {      // warm-up only: the scope's end merges the chunks into one
        FoldChunk ck{nullptr, n > FOLD_CHUNK_MIN ? n : FOLD_CHUNK_MIN};
        if (hipMalloc(reinterpret_cast<void**>(&ck.p), ck.n * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        ++g_fold.n_alloc;
        g_fold.chunks.push_back(ck);
        g_fold.used = 0;
    }
    float* p = g_fold.chunks.back().p + g_fold.used;
    g_fold.used += n;
    return p;
}

bool morec_fold_defer(const float* src, float* dst, size_t n, int cnt, size_t stride, int rpb, hipStream_t s) {
    std::lock_guard<std::mutex> lock(g_fold.mu);
    if (!g_fold.open || g_fold.producer != s) return false;
    if (n == 0 || cnt <= 0) return true;
    if (n > 0xffffffffu || stride > 0xffffffffu) return false;      // outside the job record: launched in place
    g_fold.queue.push_back(FoldJob{src, dst, (unsigned)n, (unsigned)cnt, (unsigned)stride, (unsigned)rpb, 0u, 0u});
    ++g_fold.n_jobs;
    return true;
}

extern "C" int morec_fold_defer_begin(void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!tuning().fold_defer || !morec_deterministic()) return MOREC_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    if (cap != hipStreamCaptureStatusNone) return MOREC_OK;      // a captured step keeps its folds in place
    std::lock_guard<std::mutex> lock(g_fold.mu);
    if (g_fold.open) return g_fold.producer == s ? MOREC_OK : MOREC_E_UNSUPPORTED;      // one scope per process
    g_fold.open = true;
    g_fold.producer = s;
    return MOREC_OK;
}

extern "C" int morec_fold_defer_active(void) {
    std::lock_guard<std::mutex> lock(g_fold.mu);
    return g_fold.open ? 1 : 0;
}

extern "C" int morec_fold_flush(void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lock(g_fold.mu);
    const std::vector<FoldJob>& q = g_fold.queue;
    size_t i = 0;
    while (i < q.size()) {
        FoldBatch batch;
        batch.n_jobs = 0;
        batch.pad_ = 0;
        unsigned blocks = 0;
        for (; i < q.size() && batch.n_jobs < FOLD_MAX_JOBS; ++i) {
            bool overlap = false;      // jobs that add into the same gradient run in queue order: the later one opens the next launch
            for (int k = 0; k < batch.n_jobs && !overlap; ++k)
                overlap = q[i].dst < batch.job[k].dst + batch.job[k].n && batch.job[k].dst < q[i].dst + q[i].n;
            if (overlap) break;
            FoldJob& j = batch.job[batch.n_jobs++];
            j = q[i];
            j.blk0 = blocks;
            blocks += (j.n + 15) / 16;
        }
        hipLaunchKernelGGL(fold_batch_kernel, dim3(blocks), dim3(256), 0, s, batch);
        ++g_fold.n_launch;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { g_fold.queue.clear(); return (int)e; }
    }
    g_fold.queue.clear();
    return MOREC_OK;
}

extern "C" int morec_fold_defer_end(void) {
    std::lock_guard<std::mutex> lock(g_fold.mu);
    if (!g_fold.open) return MOREC_OK;
    g_fold.open = false;
    g_fold.producer = nullptr;
    g_fold.queue.clear();      // (non-empty only when the caller abandons a step)
    g_fold.used = 0;
    if (g_fold.chunks.size() > 1) {      // warm-up: one chunk of the step's size (+ 25 %) from here on
        size_t total = 0;
        for (const FoldChunk& ck : g_fold.chunks) total += ck.n;
        (void)hipDeviceSynchronize();
        for (const FoldChunk& ck : g_fold.chunks) (void)hipFree(ck.p);
        g_fold.chunks.clear();
        FoldChunk ck{nullptr, total + total / 4};
        if (hipMalloc(reinterpret_cast<void**>(&ck.p), ck.n * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return (int)hipErrorOutOfMemory; }
        ++g_fold.n_alloc;
        g_fold.chunks.push_back(ck);
    }
    return MOREC_OK;
}

extern "C" int morec_fold_stats(unsigned long long* out4) {
    if (!out4) return MOREC_E_ARG;
    std::lock_guard<std::mutex> lock(g_fold.mu);
    size_t cap = 0;
    for (const FoldChunk& ck : g_fold.chunks) cap += ck.n;
    out4[0] = g_fold.n_alloc;
    out4[1] = (unsigned long long)cap * sizeof(float);
    out4[2] = g_fold.n_jobs;
    out4[3] = g_fold.n_launch;
    return MOREC_OK;
}

// `waiting` will not run anything issued after this call before everything issued to `signal` so far has finished: hipEventRecord +
// hipStreamWaitEvent on an event of a process-wide ring (256 entries, created on first use on the calling thread's device; re-recording an
// event that an earlier wait captured is well defined: the wait refers to the record that was current when it was issued).  What
// torch.cuda.Stream.wait_stream does, in ONE foreign call on raw handles -- the weight-gradient stream is ordered behind the backward chain
// once per dW launch (17 ... 57 times per step), and on the launch-bound configurations the host path IS the step time.  Capturable.
extern "C" int morec_stream_wait_stream(void* waiting, void* signal) {
    static hipEvent_t ring[256];
    static std::atomic<unsigned> next{0};
    static const hipError_t made = [] {
        for (auto& e : ring) {
            const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (rc != hipSuccess) return rc;
        }
        return hipSuccess;
    }();
    if (made != hipSuccess) return (int)made;
    hipEvent_t e = ring[next.fetch_add(1u, std::memory_order_relaxed) & 255u];
    hipError_t rc = hipEventRecord(e, reinterpret_cast<hipStream_t>(signal));
    if (rc != hipSuccess) return (int)rc;
    rc = hipStreamWaitEvent(reinterpret_cast<hipStream_t>(waiting), e, 0);
    return rc == hipSuccess ? MOREC_OK : (int)rc;
}

// Probe: (a) MFMA fragment/accumulator layouts with recognisable integer data, (b) what each lane of
// ds_read_b64_tr_b16 receives when lane l supplies address base + 8*l over an LDS image lds16[x] = x.
// out[0..255]     : 16x16x32 bf16: D = A.B with A[i][k] = (k == i) ? 1 : 0 for i<16 (k<16), B[k][j] = 16*k + j
//                   (assumed layouts: lane l gives row/col l&15, k = 8*(l>>4)+e) -> out[l*4+r] should be
//                   D[(l>>4)*4+r][l&15] = 16*((l>>4)*4+r) + (l&15)
// out[256..511]   : 16x16x4 f32 with the same test (k < 4 only -> rows 0..3 nonzero)
// out[512..767]   : tr_b16 values, 4 per lane
__global__ void probe_kernel(int32_t* out) {
    __shared__ __attribute__((aligned(16))) unsigned short lds16[1024];
    const int l = threadIdx.x;
    for (int i = l; i < 1024; i += 64) lds16[i] = (unsigned short)i;
    __syncthreads();
    {
        bf16x8_t a, b;
        for (int e = 0; e < 8; ++e) {
            const int k = 8 * (l >> 4) + e;
            const float av = (k == (l & 15)) ? 1.f : 0.f;                    // A[i = l&15][k]
            const float bv = (k < 16) ? (float)(16 * k + (l & 15)) : 0.f;    // B[k][j = l&15]
            a[e] = (__bf16)av;
            b[e] = (__bf16)bv;
        }
        f32x4_t c = {0.f, 0.f, 0.f, 0.f};
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
        for (int r = 0; r < 4; ++r) out[l * 4 + r] = (int32_t)c[r];
    }
    {
        const int k = l >> 4;
        const float av = (k == (l & 15)) ? 1.f : 0.f;
        const float bv = (float)(16 * k + (l & 15));
        f32x4_t c = {0.f, 0.f, 0.f, 0.f};
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c, 0, 0, 0);
        for (int r = 0; r < 4; ++r) out[256 + l * 4 + r] = (int32_t)c[r];
    }
    {
        uint64_t v;
        const uint32_t addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned short*)lds16 + 8u * l;
        asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
        for (int r = 0; r < 4; ++r) out[512 + l * 4 + r] = (int32_t)((v >> (16 * r)) & 0xffffu);
    }
}

extern "C" int morec_probe(int32_t* out, void* stream) {
    if (!out) return MOREC_E_ARG;
    hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), out);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// test hook: the keep-mask the kernels derive from (p, seed) for element indices 0 .. n-1
__global__ void drop_mask_kernel(uint8_t* out, size_t n, DropRng d) {
    d = drop_resolve(d);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = drop_keep(d, i) ? 1 : 0;
}
extern "C" int morec_dropout_keep_mask(uint8_t* out, size_t n, float p, uint64_t seed, void* stream) {
    if (!out || p < 0.f || p >= 1.f) return MOREC_E_ARG;
    if (n == 0) return MOREC_OK;
    hipLaunchKernelGGL(drop_mask_kernel, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), out, n, make_drop(p, seed));
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
