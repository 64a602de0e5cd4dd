// hutk_features.hip -- per-token features that need the text's word split: word ids.
//
// The word of a token is a rank in the word-start bitmap that hutk_pretokenize_batch_device writes (bit p: a word starts
// at byte p of the packed text) with the per-word prefix counts of hutk_pretokenize_starts_device's counting call:
//   word_id = (set bits at positions base .. base + span_start) - 1,   base: the text offset of the token's document,
// which is one or two loads and a population count.  ONE pass over the ids (k_word_ids): a workgroup takes a tile of
// WI_TILE ids, one wavefront finds the document of the tile's first id with one search, the documents that start inside
// the tile mark their first id in LDS, and a running maximum over the marks gives every id its document.  No id searches
// the offsets.  The spans are verified, not trusted: a token that holds a word start strictly inside it was made under
// another split and marks its document HUTK_DOC_SPAN_MISMATCH.
#include <string>

#include "hutk_host.h"
#include "hutk_wave.h"

namespace {

constexpr int WI_THREADS = 256, WI_PER = 8, WI_TILE = WI_THREADS * WI_PER;

struct WordArgs {
    const uint32_t* bits;     // [n_bytes / 32 + 1 and padding]
    const int64_t* before;    // [n_bytes / 32 + 2]: set bits below word w
    const int64_t* text_offs; // [n_docs + 1]
    const void* spans;        // [n_ids][2], bytes from the document's start
    const int64_t* id_offs;   // [n_docs + 1]
    int64_t n_docs, n_bytes, n_ids;
    int32_t* out;
    int32_t* status;
    int32_t* err;
};

__device__ __forceinline__ void note_error(int32_t* err, int code) {
    if (err) atomicCAS(err, 0, code);
}

// set bits at positions 0 .. p, and at positions 0 .. p - 1 (p <= n_bytes: the caller's check)
__device__ __forceinline__ int64_t rank_incl(const WordArgs& A, int64_t p) {
    return A.before[p >> 5] + __popc(A.bits[p >> 5] & ((2u << (p & 31)) - 1u));
}
__device__ __forceinline__ int64_t rank_excl(const WordArgs& A, int64_t p) {
    return A.before[p >> 5] + __popc(A.bits[p >> 5] & ((1u << (p & 31)) - 1u));
}

template <class T>
__global__ __launch_bounds__(WI_THREADS) void k_word_ids(const WordArgs A) {
    __shared__ __attribute__((aligned(16))) int32_t s_mark[WI_TILE];  // (document - d0) at the first id of a document that starts in the tile
    __shared__ int32_t s_wmax[WI_THREADS / 64];
    __shared__ int64_t s_d0;
    // nothing is read through offsets that do not describe the buffers, and nothing is written
    if (A.id_offs[0] != 0 || A.id_offs[A.n_docs] != A.n_ids || A.text_offs[0] < 0 || A.text_offs[A.n_docs] > A.n_bytes) {
        if (blockIdx.x == 0 && threadIdx.x == 0) note_error(A.err, HUTK_E_ARG);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * WI_TILE;
    const int64_t t1 = t0 + WI_TILE < A.n_ids ? t0 + WI_TILE : A.n_ids;
    for (int i = tid; i < WI_TILE; i += WI_THREADS) s_mark[i] = 0;
    if (tid < 64) {  // the last document whose ids begin at or before the tile's first: one search
        const int64_t d = hutk::wave_count_leading(A.n_docs, [&](int64_t j) { return A.id_offs[j] <= t0; }) - 1;
        if (tid == 0) s_d0 = d < 0 ? 0 : d;
    }
    __syncthreads();
    const int64_t d0 = s_d0;
    // the documents that start inside the tile; of several at one place (empty ones) the last holds the id
    for (int64_t j = d0 + 1 + tid; j < A.n_docs; j += WI_THREADS) {
        const int64_t o = A.id_offs[j];
        if (o >= t1) break;
        if (o > t0) atomicMax(&s_mark[o - t0], (int32_t)(j - d0));
    }
    __syncthreads();
    // running maximum of the marks: the document of every id, less d0
    int32_t m[WI_PER];
    {
        const int4 lo = *reinterpret_cast<const int4*>(&s_mark[tid * WI_PER]);
        const int4 hi = *reinterpret_cast<const int4*>(&s_mark[tid * WI_PER + 4]);
        m[0] = lo.x, m[1] = lo.y, m[2] = lo.z, m[3] = lo.w, m[4] = hi.x, m[5] = hi.y, m[6] = hi.z, m[7] = hi.w;
    }
#pragma unroll
    for (int e = 1; e < WI_PER; e++) m[e] = m[e] > m[e - 1] ? m[e] : m[e - 1];
    int32_t run = m[WI_PER - 1];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t p = __shfl_up(run, off);
        if (lane >= off) run = p > run ? p : run;
    }
    if (lane == 63) s_wmax[wave] = run;
    int32_t enter = __shfl_up(run, 1);  // what enters this thread's ids
    if (lane == 0) enter = 0;
    __syncthreads();
    for (int u = 0; u < wave; u++) enter = s_wmax[u] > enter ? s_wmax[u] : enter;

    const T* sp = static_cast<const T*>(A.spans);
    int64_t doc = -1, base = 0, end = 0, base_rank = 0;
    bool doc_ok = false;
#pragma unroll
    for (int e = 0; e < WI_PER; e++) {
        const int64_t k = t0 + tid * WI_PER + e;
        if (k >= t1) break;
        const int64_t d = d0 + (m[e] > enter ? m[e] : enter);
        if (d != doc) {  // the walk: a document's offsets and the rank of its first byte are read once per thread
            doc = d;
            base = A.text_offs[doc];
            end = A.text_offs[doc + 1];
            doc_ok = base >= 0 && base <= end && end <= A.n_bytes;
            base_rank = doc_ok ? rank_excl(A, base) : 0;
        }
        const int64_t a = sp[2 * k], b = sp[2 * k + 1];
        int32_t word = -1;
        if (!doc_ok || a < 0 || b < a || b > end - base) note_error(A.err, HUTK_E_ARG);  // (spans of another text)
        else {
            // (an empty span at the document's end belongs to its last word: the bit at `end` is the next document's)
            const int64_t at = a < end - base ? rank_incl(A, base + a) : rank_excl(A, base + a);
            word = (int32_t)(at - base_rank - 1);
            if (b > a + 1 && rank_incl(A, base + b - 1) != at) {  // a word starts strictly inside the token
                if (A.status) A.status[doc] = HUTK_DOC_SPAN_MISMATCH;
                note_error(A.err, HUTK_E_UNSUPPORTED);
            }
        }
        A.out[k] = word;
    }
}

bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

extern "C" {

int hutk_debug_word_ids_tile(void) { return WI_TILE; }

int hutk_token_word_ids_device(const uint32_t* d_word_bits, const int64_t* d_before, const int64_t* d_offsets, int64_t n_docs,
                               int64_t n_bytes, const void* d_spans, int span_width, const int64_t* d_id_offsets,
                               int64_t n_ids, int32_t* d_word_ids, int32_t* d_status, int32_t* d_err, void* hip_stream) {
    if (n_docs < 0 || n_bytes < 0 || n_ids < 0 || (span_width != 4 && span_width != 8) || n_docs >= INT32_MAX)
        return hutk::api_set_error(HUTK_E_ARG, "hutk_token_word_ids_device: bad arguments (span_width is 4 or 8)");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return hutk::api_set_error(HUTK_E_DEVICE, "hutk_token_word_ids_device: no HIP device");
    if (!d_word_bits || !d_before || !d_offsets || !d_id_offsets || (n_ids > 0 && (!d_spans || !d_word_ids)))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_token_word_ids_device: a buffer is NULL");
    if (!aligned_to(d_word_bits, 4) || !aligned_to(d_before, 8) || !aligned_to(d_offsets, 8) || !aligned_to(d_id_offsets, 8) ||
        !aligned_to(d_spans, (uintptr_t)span_width) || !aligned_to(d_word_ids, 4) || !aligned_to(d_status, 4))
        return hutk::api_set_error(HUTK_E_ARG, "hutk_token_word_ids_device: a buffer is not aligned to its elements");
    const int64_t blocks = (n_ids + WI_TILE - 1) / WI_TILE;
    if (blocks > INT32_MAX) return hutk::api_set_error(HUTK_E_UNSUPPORTED, "hutk_token_word_ids_device: the batch is too large for one launch");
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_err) HUTK_HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    if (d_status && n_docs > 0) HUTK_HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n_docs * sizeof(int32_t), st));
    // (with no ids one workgroup still checks the offsets)
    const WordArgs a{d_word_bits, d_before, d_offsets, d_spans, d_id_offsets, n_docs, n_bytes, n_ids, d_word_ids, d_status, d_err};
    const dim3 grid((unsigned)(blocks > 0 ? blocks : 1)), block(WI_THREADS);
    if (span_width == 4) hipLaunchKernelGGL(k_word_ids<int32_t>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_word_ids<int64_t>, grid, block, 0, st, a);
    HUTK_HIP_TRY(hipGetLastError());
    return HUTK_OK;
}

}  // extern "C"
