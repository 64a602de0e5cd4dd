// hutk_normalize.hip -- Unicode normalisation (NFC, NFD, NFKC, NFKD) of a packed batch on the GPU, in front of the
// encoders: (uint8 bytes, int64 offsets[n + 1]) in, the same pair out (include/hutoken_amd.h).
// The UTF-8 rule, the segment rule and the per-segment normaliser are hutk_norm.h, shared with the CPU check; this file
// is the chunking, the placement and the C entry points.
//
//   k_norm_check   the offsets describe the bytes (else HUTK_E_ARG and nothing else runs)
//   k_norm_sizes   one workgroup per chunk of CHUNK_BYTES, one lane per slice of 16 bytes.  The byte test first: no byte
//                  at or above the form's first unstable lead byte in the chunk and at the character behind it -> the
//                  chunk is CLEAN, its size is its input size, no table is touched.  Otherwise every lane counts the
//                  output of the segments that start in its slice (slice_run); a workgroup scan gives the chunk's size
//                  and the chunk-local place of every document that starts in it; changed[] is set.
//   k_norm_scan    exclusive scan of the chunk sizes (one workgroup, 16 K chunks a round)
//   k_norm_docs    out_offsets = chunk base + chunk-local place; the two totals
//   k_norm_write   a clean chunk is a wide copy; a dirty one counts again, scans and writes from every lane's own place
//
// The sizes call runs the first four, the write call the last one from the chunk state the sizes call left in the
// normaliser's workspace.  Neither synchronises.
#include <mutex>
#include <string>
#include <vector>

#include "hutk_host.h"
#include "hutk_norm.h"
#include "hutk_wave.h"

namespace {

namespace N = hutk::norm;

constexpr int TB = N::CHUNK_SLICES;  // 256 lanes: a slice each
static_assert(TB == 256 && N::SLICE_BYTES == 16, "a lane loads its slice as one 16-byte word");
constexpr uint32_t ST_CLEAN = 1u << 8;  // chunk state: the spill at its front | ST_CLEAN

struct NormArgs {
    N::Tables T;
    N::Text x;
    int64_t n_chunks;
    uint8_t* out;
    int64_t out_cap;
    int64_t* out_offs;
    uint8_t* changed;
    int64_t* totals;
    int64_t* chunk_base;    // [n_chunks + 1] sizes, then their exclusive scan and the total
    uint32_t* chunk_state;  // [n_chunks + 1]
    int32_t* err;
    int32_t* ok;
    int32_t wide;           // bytes is 16-byte aligned: a slice is one load
};

__device__ __forceinline__ void note_error(int32_t* err, int code) {
    if (err) atomicCAS(err, 0, code);
}

__global__ __launch_bounds__(TB) void k_norm_check(const NormArgs a) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    bool bad = false;
    if (i < a.x.n_docs) bad = a.x.offs[i + 1] < a.x.offs[i] || a.x.offs[i] < 0 || a.x.offs[i + 1] > a.x.n_bytes;
    if (i == 0) bad = bad || a.x.offs[0] != 0 || a.x.offs[a.x.n_docs] != a.x.n_bytes;
    if (bad) {
        *a.ok = 0;
        note_error(a.err, HUTK_E_ARG);
    }
}

// any byte of the dword at or above t (t >= 0x80)
__device__ __forceinline__ bool any_byte_ge(uint32_t v, uint32_t t) {
    return (v & ((v & 0x7F7F7F7Fu) + (256u - t) * 0x01010101u) & 0x80808080u) != 0;
}

// the lane's slice has a byte at or above the form's first unstable lead byte
__device__ __forceinline__ bool slice_dirty(const NormArgs& a, int64_t at, int64_t c1) {
    if (at >= c1) return false;
    if (a.wide && at + N::SLICE_BYTES <= c1) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.x.bytes + at);
        return any_byte_ge(v.x, a.x.lead) || any_byte_ge(v.y, a.x.lead) || any_byte_ge(v.z, a.x.lead) || any_byte_ge(v.w, a.x.lead);
    }
    bool d = false;
    for (int64_t p = at; p < at + N::SLICE_BYTES && p < c1; p++) d = d || a.x.bytes[p] >= a.x.lead;
    return d;
}

// what every kernel of a chunk starts with: its byte range, the documents that start in it, the spills at both edges
struct ChunkInfo {
    int64_t c0, c1, dlo, dhi;
    int sp0, sp1;
};
__device__ __forceinline__ void chunk_info(const NormArgs& a, int64_t k, int64_t* s_doc, int* s_sp, ChunkInfo& ci) {
    ci.c0 = k * N::CHUNK_BYTES;
    ci.c1 = ci.c0 + N::CHUNK_BYTES < a.x.n_bytes ? ci.c0 + N::CHUNK_BYTES : a.x.n_bytes;
    if (threadIdx.x < 128) {  // two wavefronts side by side: the front edge and the back edge
        const int64_t edge = threadIdx.x < 64 ? ci.c0 : ci.c1;
        // the first document at or after the edge (N::first_doc_at_or_after is the same function for one caller)
        const int64_t d = hutk::wave_count_leading(a.x.n_docs, [&](int64_t i) { return a.x.offs[i] < edge; });
        if ((threadIdx.x & 63) == 0) {
            s_doc[threadIdx.x >> 6] = d;
            s_sp[threadIdx.x >> 6] = N::edge_spill(a.x, edge, d);
        }
    }
    __syncthreads();
    ci.dlo = s_doc[0], ci.dhi = s_doc[1], ci.sp0 = s_sp[0], ci.sp1 = s_sp[1];
}

__global__ __launch_bounds__(TB) void k_norm_sizes(const NormArgs a) {
    __shared__ int64_t s_doc[2], s_part[TB / 64], s_excl[TB];
    __shared__ int s_sp[2];
    __shared__ uint16_t s_emit[N::CHUNK_BYTES];  // bytes a lane has put out before the segment that starts at this byte
    if (!*a.ok) return;
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x;
    ChunkInfo ci;
    chunk_info(a, k, s_doc, s_sp, ci);
    const int64_t at = ci.c0 + (int64_t)tid * N::SLICE_BYTES;
    const bool high = slice_dirty(a, at, ci.c1);
    bool dirty = high;
    if (tid == 0) dirty = dirty || (ci.c1 + ci.sp1 < a.x.n_bytes && a.x.bytes[ci.c1 + ci.sp1] >= a.x.lead);
    if (!__syncthreads_or(dirty)) {
        if (tid == 0) {
            a.chunk_base[k] = (ci.c1 + ci.sp1) - (ci.c0 + ci.sp0);
            a.chunk_state[k] = (uint32_t)ci.sp0 | ST_CLEAN;
        }
        for (int64_t d = ci.dlo + tid; d < ci.dhi; d += TB) a.out_offs[d] = a.x.offs[d] - (ci.c0 + ci.sp0);
        return;
    }
    N::CountSink sink;
    if (at < ci.c1) {
        const int64_t e = at + N::SLICE_BYTES < ci.c1 ? at + N::SLICE_BYTES : ci.c1;
        N::slice_run(a.T, a.x, N::doc_of_byte(a.x.offs, ci.dlo, ci.dhi, at), at, e, high, sink,
                     [&](int64_t p, int64_t before) { s_emit[p - ci.c0] = (uint16_t)before; }, a.changed);
    }
    int64_t total;
    s_excl[tid] = hutk::block_excl(sink.pos, s_part, total);
    __syncthreads();
    if (tid == 0) {
        a.chunk_base[k] = total;
        a.chunk_state[k] = (uint32_t)ci.sp0;
    }
    for (int64_t d = ci.dlo + tid; d < ci.dhi; d += TB) {  // (a document start is a segment start: its s_emit is written)
        const int64_t i = a.x.offs[d] - ci.c0;
        a.out_offs[d] = s_excl[i / N::SLICE_BYTES] + s_emit[i];
    }
}

constexpr int SCAN_TB = 1024, SCAN_PER = 16;
__global__ __launch_bounds__(SCAN_TB) void k_norm_scan(int64_t* v, int64_t n, const int32_t* ok) {
    __shared__ int64_t s_part[SCAN_TB / 64];
    if (!*ok) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    for (int64_t at = 0; at < n; at += SCAN_TB * SCAN_PER) {
        const int64_t i0 = at + (int64_t)tid * SCAN_PER;
        int64_t x[SCAN_PER], sum = 0;
#pragma unroll
        for (int j = 0; j < SCAN_PER; j++) {
            x[j] = i0 + j < n ? v[i0 + j] : 0;
            sum += x[j];
        }
        int64_t incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t p = __shfl_up(incl, off);
            if (lane >= off) incl += p;
        }
        if (lane == 63) s_part[w] = incl;
        __syncthreads();
        int64_t before = carry + incl - sum, total = 0;
        for (int u = 0; u < SCAN_TB / 64; u++) {
            if (u < w) before += s_part[u];
            total += s_part[u];
        }
#pragma unroll
        for (int j = 0; j < SCAN_PER; j++) {
            if (i0 + j < n) v[i0 + j] = before;
            before += x[j];
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) v[n] = carry;
}

__global__ __launch_bounds__(TB) void k_norm_docs(const NormArgs a) {
    __shared__ int64_t s_part[TB / 64];
    if (!*a.ok) return;
    const int64_t d = (int64_t)blockIdx.x * TB + threadIdx.x;
    const int64_t total = a.chunk_base[a.n_chunks];
    int64_t mine = 0;
    if (d < a.x.n_docs) {
        const int64_t o = a.x.offs[d];
        a.out_offs[d] = o >= a.x.n_bytes ? total : a.chunk_base[o / N::CHUNK_BYTES] + a.out_offs[d];
        mine = a.changed[d] != 0;
    }
    int64_t sum;
    (void)hutk::block_excl(mine, s_part, sum);
    if (threadIdx.x == 0) {
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 1), (unsigned long long)sum);
        if (blockIdx.x == 0) {
            a.out_offs[a.x.n_docs] = total;
            a.totals[0] = total;
        }
    }
}

__global__ __launch_bounds__(TB) void k_norm_write(const NormArgs a) {
    __shared__ int64_t s_doc[2], s_part[TB / 64];
    __shared__ int s_sp[2];
    if (!*a.ok) return;
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x;
    if (a.chunk_base[a.n_chunks] > a.out_cap) {  // nothing is written into a buffer the text does not fit
        if (k == 0 && tid == 0) note_error(a.err, HUTK_E_CAPACITY);
        return;
    }
    const int64_t base = a.chunk_base[k];
    const uint32_t st = a.chunk_state[k];
    if (st & ST_CLEAN) {
        const uint8_t* src = a.x.bytes + k * N::CHUNK_BYTES + (st & 0xFFu);
        uint8_t* dst = a.out + base;
        const int64_t n = a.chunk_base[k + 1] - base;
        if (src + n > a.x.bytes + a.x.n_bytes || base + n > a.out_cap) return;  // (a state that is not this batch's)
        int64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
        if (((reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src)) & 15) != 0 || head > n) head = n;
        for (int64_t i = tid; i < head; i += TB) dst[i] = src[i];
        const int64_t words = (n - head) >> 4;
        for (int64_t i = tid; i < words; i += TB)
            reinterpret_cast<uint4*>(dst + head)[i] = reinterpret_cast<const uint4*>(src + head)[i];
        for (int64_t i = head + (words << 4) + tid; i < n; i += TB) dst[i] = src[i];
        return;
    }
    ChunkInfo ci;
    chunk_info(a, k, s_doc, s_sp, ci);
    const int64_t at = ci.c0 + (int64_t)tid * N::SLICE_BYTES;
    const int64_t e = at + N::SLICE_BYTES < ci.c1 ? at + N::SLICE_BYTES : ci.c1;
    const int64_t d = at < ci.c1 ? N::doc_of_byte(a.x.offs, ci.dlo, ci.dhi, at) : 0;
    const bool high = slice_dirty(a, at, ci.c1);
    N::CountSink count;
    if (at < ci.c1) N::slice_run(a.T, a.x, d, at, e, high, count, [](int64_t, int64_t) {}, nullptr);
    int64_t total;
    const int64_t before = hutk::block_excl(count.pos, s_part, total);
    if (at < ci.c1 && count.pos) {
        N::WriteSink sink{a.out, a.out_cap, base + before};
        N::slice_run(a.T, a.x, d, at, e, high, sink, [](int64_t, int64_t) {}, nullptr);
    }
}

bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

struct hutk_normalizer {
    int device = 0;
    uint32_t head[N::HEADER_WORDS] = {0};
    int64_t blob_bytes = 0;
    DevBuf<uint8_t> d_blob, w_changed, s_bytes, s_out;
    DevBuf<int64_t> w_base, w_totals, s_offs, s_oo;
    DevBuf<uint32_t> w_state;
    DevBuf<int32_t> w_ok;  // [0] the batch's offsets are sound, [1] the error word of a caller that passes none
    N::Tables T{};
    // the batch whose chunk state the workspace holds (the sizes call that ran last)
    struct Key {
        int form = -1;
        const void *bytes = nullptr, *offs = nullptr;
        int64_t n_docs = -1, n_bytes = -1;
        bool operator==(const Key& o) const {
            return form == o.form && bytes == o.bytes && offs == o.offs && n_docs == o.n_docs && n_bytes == o.n_bytes;
        }
    } key;
    std::mutex mu;
    hipEvent_t ev = nullptr;  // behind the last kernel of the last call: calls share the workspace, so they are serialised
    bool ev_recorded = false;
};

extern "C" {

int hutk_debug_norm_chunk_bytes(void) { return N::CHUNK_BYTES; }

void hutk_normalizer_destroy(hutk_normalizer* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev) {
        if (h->ev_recorded) (void)hipEventSynchronize(h->ev);  // nothing is freed under a running kernel
        (void)hipEventDestroy(h->ev);
    }
    h->d_blob.release(); h->w_changed.release(); h->s_bytes.release(); h->s_out.release(); h->w_base.release();
    h->w_totals.release(); h->s_offs.release(); h->s_oo.release(); h->w_state.release(); h->w_ok.release();
    delete h;
}

int hutk_normalizer_create(hutk_normalizer** out, int device, const uint8_t* blob, int64_t n_blob_bytes) {
    if (!out) return hutk::api_set_error(HUTK_E_ARG, "hutk_normalizer_create: out is NULL");
    *out = nullptr;
    uint32_t head[N::HEADER_WORDS];
    std::string why;
    if (!N::validate_blob(blob, n_blob_bytes, head, &why)) return hutk::api_set_error(HUTK_E_VALUE, "hutk_normalizer_create: " + why);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_normalizer_create: no HIP device");
    if (device < 0) HUTK_HIP_TRY(hipGetDevice(&device));
    if (device >= n) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_normalizer_create: no such device");
    HUTK_HIP_TRY(hipSetDevice(device));
    hutk_normalizer* h = new hutk_normalizer();
    h->device = device;
    h->blob_bytes = n_blob_bytes;
    for (uint32_t i = 0; i < N::HEADER_WORDS; i++) h->head[i] = head[i];
    hipError_t e = h->d_blob.reserve((size_t)n_blob_bytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_blob.p, blob, (size_t)n_blob_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->w_ok.reserve(2);
    if (e == hipSuccess) e = h->w_totals.reserve(2);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        hutk_normalizer_destroy(h);
        return hutk::api_set_error(e == hipErrorOutOfMemory ? HUTK_E_MEMORY : HUTK_E_DEVICE,
                                   std::string("hutk_normalizer_create: ") + hipGetErrorString(e));
    }
    h->T = N::tables_of(h->d_blob.p, h->head);
    *out = h;
    return HUTK_OK;
}

int hutk_normalizer_info(const hutk_normalizer* h, int64_t* out8) {
    if (!h || !out8) return hutk::api_set_error(HUTK_E_ARG, "hutk_normalizer_info: bad arguments");
    out8[0] = h->head[N::H_VERSION];
    out8[1] = h->head[N::H_UNIDATA];
    out8[2] = h->blob_bytes;
    out8[3] = N::CHUNK_BYTES;
    out8[4] = h->head[N::H_PAIRS_N];
    out8[5] = h->head[N::H_DECOMP_N];
    out8[6] = (int64_t)h->head[N::H_LEAD] | (int64_t)h->head[N::H_LEAD + 1] << 8 | (int64_t)h->head[N::H_LEAD + 2] << 16 |
              (int64_t)h->head[N::H_LEAD + 3] << 24;
    out8[7] = (int64_t)h->head[N::H_RATIO] | (int64_t)h->head[N::H_RATIO + 1] << 8 | (int64_t)h->head[N::H_RATIO + 2] << 16 |
              (int64_t)h->head[N::H_RATIO + 3] << 24;
    return HUTK_OK;
}

int hutk_normalize_batch_device(hutk_normalizer* h, int form, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                int64_t n_bytes, uint8_t* d_out, int64_t out_cap, int64_t* d_out_offsets, uint8_t* d_changed,
                                int64_t* d_totals, int32_t* d_err, void* hip_stream) {
    if (!h) return hutk::api_set_error(HUTK_E_ARG, "hutk_normalize_batch_device: the normaliser is NULL");
    if (form < 0 || form >= N::N_FORMS)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_normalize_batch_device: form must be HUTK_NFC, HUTK_NFD, HUTK_NFKC or HUTK_NFKD");
    if (n_docs < 0 || n_bytes < 0 || out_cap < 0 || !d_offsets || (n_bytes > 0 && !d_bytes))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_normalize_batch_device: bad arguments");
    const int64_t n_chunks = (n_bytes + N::CHUNK_BYTES - 1) / N::CHUNK_BYTES;
    if (n_chunks > INT32_MAX || (n_docs + TB - 1) / TB > INT32_MAX)
        return hutk::api_set_error(HUTK_E_UNSUPPORTED, "hutk_normalize_batch_device: the batch is too large for one launch");
    std::lock_guard<std::mutex> lock(h->mu);
    hutk_normalizer::Key key;
    key.form = form, key.bytes = d_bytes, key.offs = d_offsets, key.n_docs = n_docs, key.n_bytes = n_bytes;
    const bool sizes = !d_out || !(key == h->key);  // a write call without its sizes call runs that first
    if (sizes && (!d_out_offsets || !d_totals))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_normalize_batch_device: the sizes call needs d_out_offsets and d_totals (and a write call "
                                               "its sizes call, with the same batch, right before it)");
    HUTK_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (sizes) {
        HUTK_HIP_TRY(h->w_base.reserve((size_t)n_chunks + 1));
        HUTK_HIP_TRY(h->w_state.reserve((size_t)n_chunks + 1));
        if (!d_changed) HUTK_HIP_TRY(h->w_changed.reserve((size_t)n_docs + 1));
    }
    if (h->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
    NormArgs a;
    a.T = h->T;
    a.x = N::Text{d_bytes, d_offsets, n_docs, n_bytes, h->head[N::H_LEAD + form], form};
    a.n_chunks = n_chunks;
    a.out = d_out;
    a.out_cap = out_cap;
    a.out_offs = d_out_offsets;
    a.changed = d_changed ? d_changed : h->w_changed.p;
    a.totals = d_totals;
    a.chunk_base = h->w_base.p;
    a.chunk_state = h->w_state.p;
    a.err = d_err ? d_err : h->w_ok.p + 1;
    a.ok = h->w_ok.p;
    a.wide = aligned_to(d_bytes, 16);
    HUTK_HIP_TRY(hipMemsetAsync(a.err, 0, sizeof(int32_t), st));
    if (sizes) {
        h->key = hutk_normalizer::Key();
        HUTK_HIP_TRY(hipMemsetAsync(a.ok, 1, sizeof(int32_t), st));
        HUTK_HIP_TRY(hipMemsetAsync(d_totals, 0, 2 * sizeof(int64_t), st));
        if (n_docs) HUTK_HIP_TRY(hipMemsetAsync(a.changed, 0, (size_t)n_docs, st));
        HUTK_HIP_TRY(hipMemsetAsync(a.chunk_base, 0, ((size_t)n_chunks + 1) * sizeof(int64_t), st));
        hipLaunchKernelGGL(k_norm_check, dim3((unsigned)((n_docs + TB) / TB)), dim3(TB), 0, st, a);
        if (n_chunks) hipLaunchKernelGGL(k_norm_sizes, dim3((unsigned)n_chunks), dim3(TB), 0, st, a);
        hipLaunchKernelGGL(k_norm_scan, dim3(1), dim3(SCAN_TB), 0, st, a.chunk_base, n_chunks, a.ok);
        hipLaunchKernelGGL(k_norm_docs, dim3((unsigned)((n_docs + TB) / TB)), dim3(TB), 0, st, a);
        HUTK_HIP_TRY(hipGetLastError());
        h->key = key;
    }
    if (d_out && n_chunks) {
        hipLaunchKernelGGL(k_norm_write, dim3((unsigned)n_chunks), dim3(TB), 0, st, a);
        HUTK_HIP_TRY(hipGetLastError());
    }
    HUTK_HIP_TRY(hipEventRecord(h->ev, st));
    h->ev_recorded = true;
    return HUTK_OK;
}

int hutk_normalize_batch(hutk_normalizer* h, int form, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, uint8_t** out,
                         int64_t** out_offsets) {
    if (!h || !out || !out_offsets || n_docs < 0 || !offsets) return hutk::api_set_error(HUTK_E_ARG, "hutk_normalize_batch: bad arguments");
    *out = nullptr;
    *out_offsets = nullptr;
    if (form < 0 || form >= N::N_FORMS) return hutk::api_set_error(HUTK_E_ARG, "hutk_normalize_batch: form must be HUTK_NFC, HUTK_NFD, HUTK_NFKC or HUTK_NFKD");
    if (int rc = hutk::check_offsets(offsets, n_docs, true, "offsets")) return rc;
    const int64_t n_bytes = offsets[n_docs];
    if (n_bytes > 0 && !bytes) return hutk::api_set_error(HUTK_E_ARG, "hutk_normalize_batch: bytes is NULL");
    HUTK_HIP_TRY(hipSetDevice(h->device));
    {
        std::lock_guard<std::mutex> lock(h->mu);
        HUTK_HIP_TRY(h->s_bytes.reserve((size_t)n_bytes + 16));
        HUTK_HIP_TRY(h->s_offs.reserve((size_t)n_docs + 1));
        HUTK_HIP_TRY(h->s_oo.reserve((size_t)n_docs + 1));
        if (h->ev_recorded) HUTK_HIP_TRY(hipEventSynchronize(h->ev));  // (the staging buffers are the normaliser's)
        if (n_bytes) HUTK_HIP_TRY(hipMemcpy(h->s_bytes.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice));
        HUTK_HIP_TRY(hipMemcpy(h->s_offs.p, offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
    }
    int64_t totals[2] = {0, 0};
    int32_t err = 0;
    if (int rc = hutk_normalize_batch_device(h, form, h->s_bytes.p, h->s_offs.p, n_docs, n_bytes, nullptr, 0, h->s_oo.p, nullptr,
                                             h->w_totals.p, nullptr, nullptr))
        return rc;
    HUTK_HIP_TRY(hipMemcpy(totals, h->w_totals.p, sizeof(totals), hipMemcpyDeviceToHost));
    HUTK_HIP_TRY(hipMemcpy(&err, h->w_ok.p + 1, 4, hipMemcpyDeviceToHost));
    if (err) return hutk::api_set_error(err, "hutk_normalize_batch: device-side failure");
    const int64_t total = totals[0];
    HUTK_HIP_TRY(h->s_out.reserve((size_t)total + 16));
    if (int rc = hutk_normalize_batch_device(h, form, h->s_bytes.p, h->s_offs.p, n_docs, n_bytes, h->s_out.p, total, nullptr, nullptr,
                                             nullptr, nullptr, nullptr))
        return rc;
    uint8_t* ob = (uint8_t*)hutk_host_alloc((size_t)(total > 0 ? total : 1));
    int64_t* oo = (int64_t*)hutk_host_alloc((size_t)(n_docs + 1) * 8);
    if (!ob || !oo) {
        if (ob) hutk_host_free(ob);
        if (oo) hutk_host_free(oo);
        return hutk::api_set_error(HUTK_E_MEMORY, "hutk_normalize_batch: out of host memory");
    }
    hipError_t e = total ? hipMemcpy(ob, h->s_out.p, (size_t)total, hipMemcpyDeviceToHost) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(oo, h->s_oo.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        hutk_host_free(ob);
        hutk_host_free(oo);
        HUTK_HIP_TRY(e);
    }
    *out = ob;
    *out_offsets = oo;
    return HUTK_OK;
}

}  // extern "C"
