// hutk_presplit.hip -- the word split of the presets gpt2, cl100k (llama3) and qwen2 on the GPU: packed text in, the
// word-start bitmap the encoders take (BatchArgs::word_bits) out (include/hutoken_amd.h).  The
// UTF-8 rule, the classes and the split rule are hutk_presplit.h, shared with the CPU check; this file is the staging,
// the scans and the C entry points.
//
//   k_ps_check   the offsets describe the bytes (else HUTK_E_ARG and nothing else runs)
//   k_ps_maps    cl100k, qwen2: one workgroup per chunk of CHUNK_BYTES, one lane per slice of 16 bytes.  The chunk and
//                its halo are staged in LDS with 16-byte loads, every byte gets its code, every slice its two maps
//                (digit count mod 3 and swallowed newlines forward, "a newline lies ahead" backward), the workgroup
//                composes them into the chunk's
//   k_ps_scan    one workgroup: the state that enters every chunk from the left and from the right
//   k_ps_write   stages and classifies again, scans the slice maps, and every lane decides the 16 bits of its slice;
//                two lanes' bits are one 32-bit store
// gpt2 is local throughout: k_ps_check and k_ps_write only.  Nothing synchronises; every position is 64 bits wide.
#include <mutex>
#include <string>

#include "hutk_host.h"
#include "hutk_presplit.h"
#include "hutk_wave.h"

namespace {

namespace P = hutk::presplit;

constexpr int TB = P::CHUNK_BYTES / P::SLICE_BYTES;  // 256 lanes: a slice each
constexpr int WIN = P::BACK + P::CHUNK_BYTES + P::AHEAD;
constexpr int RAW_WORDS = WIN / 16 + 1;  // 16-byte words that cover the window at any alignment of the text
constexpr int CHUNK_WORDS = P::CHUNK_BYTES / 32;
constexpr int PAD_WORDS = 40;            // the bitmap has n_bytes / 32 + PAD_WORDS words (the encoders read ahead)
static_assert(TB == 256 && WIN % 32 == 0 && P::BACK % 16 == 0, "the staging below");

struct SplitArgs {
    P::Tables T;
    const uint8_t* bytes;
    const int64_t* offs;
    int64_t n_docs, n_bytes, n_chunks, n_words;
    int preset;
    uint32_t* bits;
    uint32_t* maps;   // [n_chunks] maps_pack of every chunk
    uint32_t* carry;  // [n_chunks] carry_pack: what enters the chunk
    int32_t* err;
    int32_t* ok;
};

__global__ __launch_bounds__(TB) void k_ps_check(const SplitArgs a) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    bool bad = false;
    if (i < a.n_docs) bad = a.offs[i + 1] < a.offs[i] || a.offs[i] < 0 || a.offs[i + 1] > a.n_bytes;
    if (i == 0) bad = bad || a.offs[0] != 0 || a.offs[a.n_docs] != a.n_bytes;
    if (bad) {
        *a.ok = 0;
        if (a.err) atomicCAS(a.err, 0, HUTK_E_ARG);
    }
}

struct Staged {
    P::Win W;
    int64_t c0, c1;
};

// bytes, document bits and codes of chunk k in LDS
__device__ __forceinline__ void stage(const SplitArgs& a, int64_t k, uint4* s_raw, uint32_t* s_code, uint32_t* s_doc, Staged& S) {
    const int tid = threadIdx.x;
    S.c0 = k * P::CHUNK_BYTES;
    S.c1 = S.c0 + P::CHUNK_BYTES < a.n_bytes ? S.c0 + P::CHUNK_BYTES : a.n_bytes;
    const int64_t w0 = S.c0 - P::BACK;
    const uintptr_t at = reinterpret_cast<uintptr_t>(a.bytes) + (uintptr_t)w0;
    const int sh = (int)(at & 15u);
    for (int j = tid; j < RAW_WORDS; j += TB) {  // aligned words; one that holds no byte of the batch is not read
        const int64_t lo = w0 - sh + 16 * (int64_t)j;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (lo < a.n_bytes && lo + 16 > 0) v = *reinterpret_cast<const uint4*>(at - sh + 16u * (uintptr_t)j);
        s_raw[j] = v;
    }
    for (int j = tid; j < WIN / 4; j += TB) s_code[j] = 0;
    for (int j = tid; j < WIN / 32 + 1; j += TB) s_doc[j] = 0;
    __syncthreads();
    const int64_t dlo = hutk::wave_count_leading(a.n_docs, [&](int64_t i) { return a.offs[i] < w0; });  // the first document at or after w0
    for (int64_t d = dlo + tid; d <= a.n_docs; d += TB) {
        const int64_t o = a.offs[d] - w0;
        if (o >= WIN) break;
        atomicOr(&s_doc[o >> 5], 1u << (o & 31));
    }
    __syncthreads();
    S.W = P::Win{reinterpret_cast<const uint8_t*>(s_raw) + sh, reinterpret_cast<uint8_t*>(s_code), s_doc};
    for (int s = tid; s < (P::CHUNK_BYTES + 2 * P::CLS_HALO) / 16; s += TB) {
        const int i0 = P::BACK - P::CLS_HALO + 16 * s;
        for (int i = i0; i < i0 + 16; i++)
            if (w0 + i >= 0 && w0 + i < a.n_bytes) S.W.code[i] = (uint8_t)P::classify_byte(a.T, S.W, i);
    }
    __syncthreads();
}

// What enters every lane's slice: the composition of the slices in front of it (f_before) and behind it (b_behind), and
// the chunk's two maps.  s_part: eight words of LDS.
__device__ __forceinline__ void scan_maps(uint32_t f, uint32_t b, uint32_t* s_part, uint32_t& f_before, uint32_t& b_behind,
                                          uint32_t& f_all, uint32_t& b_all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t fi = f, bi = b;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t pf = __shfl_up(fi, off), pb = __shfl_down(bi, off);
        if (lane >= off) fi = P::fmap_then(pf, fi);
        if (lane + off < 64) bi = P::bmap_then(pb, bi);
    }
    if (lane == 63) s_part[wave] = fi;
    if (lane == 0) s_part[4 + wave] = bi;
    const uint32_t fe = __shfl_up(fi, 1), be = __shfl_down(bi, 1);
    __syncthreads();
    uint32_t fp = P::FMAP_IDENT, bp = P::BMAP_IDENT;
    f_all = P::FMAP_IDENT, b_all = P::BMAP_IDENT;
#pragma unroll
    for (int u = 0; u < TB / 64; u++) {
        if (u < wave) fp = P::fmap_then(fp, s_part[u]);
        f_all = P::fmap_then(f_all, s_part[u]);
    }
#pragma unroll
    for (int u = TB / 64 - 1; u >= 0; u--) {
        if (u > wave) bp = P::bmap_then(bp, s_part[4 + u]);
        b_all = P::bmap_then(b_all, s_part[4 + u]);
    }
    f_before = lane == 0 ? fp : P::fmap_then(fp, fe);
    b_behind = lane == 63 ? bp : P::bmap_then(bp, be);
    __syncthreads();
}

__device__ __forceinline__ void slice_of(const Staged& S, int& i0, int& n) {
    const int64_t at = S.c0 + (int64_t)threadIdx.x * P::SLICE_BYTES;
    i0 = P::BACK + (int)threadIdx.x * P::SLICE_BYTES;
    n = at >= S.c1 ? 0 : S.c1 - at < P::SLICE_BYTES ? (int)(S.c1 - at) : P::SLICE_BYTES;
}

__global__ __launch_bounds__(TB) void k_ps_maps(const SplitArgs a) {
    __shared__ uint4 s_raw[RAW_WORDS];
    __shared__ uint32_t s_code[WIN / 4], s_doc[WIN / 32 + 1], s_part[8];
    if (!*a.ok) return;
    Staged S;
    stage(a, blockIdx.x, s_raw, s_code, s_doc, S);
    int i0, n;
    slice_of(S, i0, n);
    uint32_t fb, bb, f_all, b_all;
    scan_maps(P::slice_fmap(S.W, i0, i0 + n), P::slice_bmap(S.W, i0, i0 + n), s_part, fb, bb, f_all, b_all);
    if (threadIdx.x == 0) a.maps[blockIdx.x] = P::maps_pack(f_all, b_all);
}

constexpr int SCAN_TB = 1024;
__global__ __launch_bounds__(SCAN_TB) void k_ps_scan(const uint32_t* maps, uint32_t* carry, int64_t n, const int32_t* ok) {
    __shared__ uint32_t s_f[SCAN_TB], s_b[SCAN_TB];
    if (!*ok) return;
    const int tid = threadIdx.x;
    const int64_t per = (n + SCAN_TB - 1) / SCAN_TB;
    const int64_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t f = P::FMAP_IDENT, b = P::BMAP_IDENT;
    for (int64_t k = lo; k < hi; k++) f = P::fmap_then(f, maps[k] & 0xFFFFu);
    for (int64_t k = hi - 1; k >= lo; k--) b = P::bmap_then(b, maps[k] >> 16);
    s_f[tid] = f, s_b[tid] = b;
    __syncthreads();
    if (tid == 0) {  // what enters every thread's stretch (in place)
        uint32_t fs = P::F_NONE, bv = 0;
        for (int t = 0; t < SCAN_TB; t++) {
            const uint32_t m = s_f[t];
            s_f[t] = fs;
            fs = P::fmap_get(m, fs);
        }
        for (int t = SCAN_TB - 1; t >= 0; t--) {
            const uint32_t m = s_b[t];
            s_b[t] = bv;
            bv = P::bmap_get(m, bv);
        }
    }
    __syncthreads();
    uint32_t fs = s_f[tid], bv = s_b[tid];
    for (int64_t k = lo; k < hi; k++) {
        carry[k] = fs;
        fs = P::fmap_get(maps[k] & 0xFFFFu, fs);
    }
    for (int64_t k = hi - 1; k >= lo; k--) {
        carry[k] = P::carry_pack(carry[k], bv);
        bv = P::bmap_get(maps[k] >> 16, bv);
    }
}

__global__ __launch_bounds__(TB) void k_ps_write(const SplitArgs a) {
    __shared__ uint4 s_raw[RAW_WORDS];
    __shared__ uint32_t s_code[WIN / 4], s_doc[WIN / 32 + 1], s_part[8];
    __shared__ uint16_t s_bits[TB];
    if (!*a.ok) return;
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x;
    Staged S;
    stage(a, k, s_raw, s_code, s_doc, S);
    int i0, n;
    slice_of(S, i0, n);
    uint32_t fwd = P::F_NONE, ahead = 0;
    if (a.preset != P::PRESET_GPT2) {
        uint32_t fb, bb, f_all, b_all;
        scan_maps(P::slice_fmap(S.W, i0, i0 + n), P::slice_bmap(S.W, i0, i0 + n), s_part, fb, bb, f_all, b_all);
        const uint32_t in = a.carry[k];
        fwd = P::fmap_get(fb, in & 0xFFu);
        ahead = P::bmap_get(bb, in >> 8);
    }
    uint32_t bits = P::slice_starts(S.W, a.preset, i0, n, fwd, ahead);
    const int64_t end = a.n_bytes - (S.c0 + (int64_t)tid * P::SLICE_BYTES);  // the bit at n_bytes
    if (end >= 0 && end < P::SLICE_BYTES) bits |= 1u << end;
    s_bits[tid] = (uint16_t)bits;
    __syncthreads();
    const int64_t w = k * CHUNK_WORDS + tid;
    if (tid < CHUNK_WORDS && w < a.n_words) a.bits[w] = (uint32_t)s_bits[2 * tid] | (uint32_t)s_bits[2 * tid + 1] << 16;
    if (k == a.n_chunks - 1 && w + CHUNK_WORDS < a.n_words) a.bits[w + CHUNK_WORDS] = 0;  // (at most PAD_WORDS of them)
}

// positions of the set bits: k_ps_popc counts them word by word (an exclusive scan follows), k_ps_list writes them out and
// finds every document's first
constexpr int LIST_TB = 256;
__global__ __launch_bounds__(LIST_TB) void k_ps_popc(const uint32_t* bits, int64_t n_words, int64_t* before, const int32_t* ok) {
    const int64_t w = (int64_t)blockIdx.x * LIST_TB + threadIdx.x;
    if (!*ok) return;
    if (w < n_words) before[w] = __popc(bits[w]);
}
__global__ __launch_bounds__(LIST_TB) void k_ps_list(const uint32_t* bits, int64_t n_bytes, const int64_t* before, const int64_t* offs,
                                                      int64_t n_docs, int64_t* starts, int64_t* start_offs, const int32_t* ok) {
    const int64_t i = (int64_t)blockIdx.x * LIST_TB + threadIdx.x;
    if (!*ok) return;
    const int64_t n_words = n_bytes / 32 + 1;
    if (i < n_words) {
        uint32_t v = bits[i];
        if (i == n_bytes / 32) v &= (1u << (n_bytes & 31)) - 1u;  // the bit at n_bytes is no word
        int64_t at = before[i];
        while (v) {
            const int b = __ffs(v) - 1;
            starts[at++] = i * 32 + b;
            v &= v - 1;
        }
    }
    if (i <= n_docs) {  // starts before the document's first byte
        const int64_t o = offs[i];
        start_offs[i] = before[o >> 5] + __popc(bits[o >> 5] & ((1u << (o & 31)) - 1u));
    }
}

bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

struct hutk_pretokenizer {
    int device = 0;
    uint32_t head[P::HEADER_WORDS] = {0};
    int64_t blob_bytes = 0;
    DevBuf<uint8_t> d_blob;
    DevBuf<uint32_t> w_maps, w_carry;
    DevBuf<int32_t> w_ok;  // [0] the batch's offsets are sound, [1] the error word of a caller that passes none
    P::Tables T{};
    std::mutex mu;
    hipEvent_t ev = nullptr;  // behind the last kernel of the last call: calls share the workspace, so they are serialised
    bool ev_recorded = false;
};

extern "C" {

int hutk_debug_presplit_chunk_bytes(void) { return P::CHUNK_BYTES; }

void hutk_pretokenizer_destroy(hutk_pretokenizer* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev) {
        if (h->ev_recorded) (void)hipEventSynchronize(h->ev);  // nothing is freed under a running kernel
        (void)hipEventDestroy(h->ev);
    }
    h->d_blob.release(); h->w_maps.release(); h->w_carry.release(); h->w_ok.release();
    delete h;
}

int hutk_pretokenizer_create(hutk_pretokenizer** out, int device, const uint8_t* blob, int64_t n_blob_bytes) {
    if (!out) return hutk::api_set_error(HUTK_E_ARG, "hutk_pretokenizer_create: out is NULL");
    *out = nullptr;
    uint32_t head[P::HEADER_WORDS];
    std::string why;
    if (!P::validate_blob(blob, n_blob_bytes, head, &why)) return hutk::api_set_error(HUTK_E_VALUE, "hutk_pretokenizer_create: " + why);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_pretokenizer_create: no HIP device");
    if (device < 0) HUTK_HIP_TRY(hipGetDevice(&device));
    if (device >= n) return hutk::api_set_error(HUTK_E_DEVICE, "hutk_pretokenizer_create: no such device");
    HUTK_HIP_TRY(hipSetDevice(device));
    hutk_pretokenizer* h = new hutk_pretokenizer();
    h->device = device;
    h->blob_bytes = n_blob_bytes;
    for (uint32_t i = 0; i < P::HEADER_WORDS; i++) h->head[i] = head[i];
    hipError_t e = h->d_blob.reserve((size_t)n_blob_bytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_blob.p, blob, (size_t)n_blob_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->w_ok.reserve(2);
    // (no split yet: a bitmap given to hutk_pretokenize_starts_device is the caller's own and counts as sound)
    if (e == hipSuccess) e = hipMemset(h->w_ok.p, 1, sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->w_ok.p + 1, 0, sizeof(int32_t));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        hutk_pretokenizer_destroy(h);
        return hutk::api_set_error(e == hipErrorOutOfMemory ? HUTK_E_MEMORY : HUTK_E_DEVICE,
                                   std::string("hutk_pretokenizer_create: ") + hipGetErrorString(e));
    }
    h->T = P::tables_of(h->d_blob.p, h->head);
    *out = h;
    return HUTK_OK;
}

int hutk_pretokenize_batch_device(hutk_pretokenizer* h, int preset, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs,
                                  int64_t n_bytes, uint32_t* d_word_bits, int32_t* d_err, void* hip_stream) {
    if (!h) return hutk::api_set_error(HUTK_E_ARG, "hutk_pretokenize_batch_device: the pre-tokeniser is NULL");
    if (preset < 0 || preset >= P::N_PRESETS)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pretokenize_batch_device: preset must be HUTK_PRESPLIT_GPT2, _CL100K or _QWEN2");
    if (n_docs < 0 || n_bytes < 0 || !d_offsets || !d_word_bits || (n_bytes > 0 && !d_bytes) || !aligned_to(d_word_bits, 4) ||
        !aligned_to(d_offsets, 8))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pretokenize_batch_device: bad arguments");
    const int64_t n_chunks = n_bytes / P::CHUNK_BYTES + 1;  // (the chunk that holds the bit at n_bytes may hold no byte)
    if (n_chunks > INT32_MAX || (n_docs + TB) / TB > INT32_MAX)
        return hutk::api_set_error(HUTK_E_UNSUPPORTED, "hutk_pretokenize_batch_device: the batch is too large for one launch");
    std::lock_guard<std::mutex> lock(h->mu);
    HUTK_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const bool carries = preset != P::PRESET_GPT2;
    if (carries) {
        HUTK_HIP_TRY(h->w_maps.reserve((size_t)n_chunks));
        HUTK_HIP_TRY(h->w_carry.reserve((size_t)n_chunks));
    }
    if (h->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
    SplitArgs a;
    a.T = h->T;
    a.bytes = d_bytes;
    a.offs = d_offsets;
    a.n_docs = n_docs, a.n_bytes = n_bytes, a.n_chunks = n_chunks, a.n_words = n_bytes / 32 + PAD_WORDS;
    a.preset = preset;
    a.bits = d_word_bits;
    a.maps = h->w_maps.p;
    a.carry = h->w_carry.p;
    a.err = d_err ? d_err : h->w_ok.p + 1;
    a.ok = h->w_ok.p;
    HUTK_HIP_TRY(hipMemsetAsync(a.err, 0, sizeof(int32_t), st));
    HUTK_HIP_TRY(hipMemsetAsync(a.ok, 1, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_ps_check, dim3((unsigned)((n_docs + TB) / TB)), dim3(TB), 0, st, a);
    if (carries) {
        hipLaunchKernelGGL(k_ps_maps, dim3((unsigned)n_chunks), dim3(TB), 0, st, a);
        hipLaunchKernelGGL(k_ps_scan, dim3(1), dim3(SCAN_TB), 0, st, a.maps, a.carry, n_chunks, a.ok);
    }
    hipLaunchKernelGGL(k_ps_write, dim3((unsigned)n_chunks), dim3(TB), 0, st, a);
    HUTK_HIP_TRY(hipGetLastError());
    HUTK_HIP_TRY(hipEventRecord(h->ev, st));
    h->ev_recorded = true;
    return HUTK_OK;
}

int hutk_pretokenize_starts_device(hutk_pretokenizer* h, const uint32_t* d_word_bits, const int64_t* d_offsets, int64_t n_docs,
                                   int64_t n_bytes, int64_t* d_before, int64_t* d_starts, int64_t* d_start_offsets, void* hip_stream) {
    if (!h || !d_word_bits || !d_offsets || !d_before || (d_starts && !d_start_offsets) || n_docs < 0 || n_bytes < 0)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_pretokenize_starts_device: bad arguments");
    const int64_t n_words = n_bytes / 32 + 1;
    const int64_t n_blocks = ((n_words > n_docs + 1 ? n_words : n_docs + 1) + LIST_TB - 1) / LIST_TB;
    if (n_blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, "hutk_pretokenize_starts_device: the batch is too large for one launch");
    std::lock_guard<std::mutex> lock(h->mu);
    HUTK_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (!d_starts) {  // the counting call: d_before[w] = set bits below word w, d_before[n_words] = all of them
        hipLaunchKernelGGL(k_ps_popc, dim3((unsigned)((n_words + LIST_TB - 1) / LIST_TB)), dim3(LIST_TB), 0, st, d_word_bits, n_words, d_before,
                           h->w_ok.p);
        HUTK_HIP_TRY(hipGetLastError());
        hutk::launch_scan_i64(d_before, n_words, st);
        return HUTK_OK;
    }
    hipLaunchKernelGGL(k_ps_list, dim3((unsigned)n_blocks), dim3(LIST_TB), 0, st, d_word_bits, n_bytes, d_before, d_offsets, n_docs, d_starts,
                       d_start_offsets, h->w_ok.p);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

}  // extern "C"
