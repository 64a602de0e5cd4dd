// hutk_unigram_train.h -- fitting a Unigram vocabulary on the GPU (include/hutoken_amd.h states the rule; DESIGN.md
// section 8n.2): the kernels of the E-step, the M-step and the prune, and their C entry points.  hutk_unigram.hip includes
// it behind its own kernels, as hutk_kernels.hip includes hutk_exc.h: the check, the flags, the fold, the chunks, the word
// queue, the groups of 8 lanes, the trip over 8 lengths and the handle are that file's and are used as they stand.
//
//   k_ug_estep          in k_ug_sample's place: a group sums a word's lattice from its end (bwd: the sampler's filter, in a
//                       ring of LDS and, for a word that does not fit it, in the per-byte workspace as well), then walks
//                       the starts in rising order with fwd in a SECOND ring, runs the trips of every start again and adds
//                       exp(fwd[s] + x + bwd[e] - Z) of every candidate to its piece's expected count
//   k_ug_mstep_*        the survivors' sum, then digamma(count) - digamma(sum), the dead set, the alive count and the
//                       lowest score alive, from which the unknown edge's score follows
//   k_ug_lattice_train  k_ug_lattice's body over lattice_word<true>: dead pieces are no candidates; over the corpus for
//                       the prune's histogram, and over the KEY BLOB ITSELF -- every key a document of one word, folded
//                       already -- with the spanning edge barred for the alternatives
//   k_ug_hist           the ids of the best path counted per piece
//   k_ug_alt_class, k_ug_vsum, k_ug_loss   a lane a table slot: the class of a piece, the histogram's sum, the loss
//
// LDS and occupancy of k_ug_estep.  k_ug_sample's workgroup holds 32 KiB of rings and 8 KiB of word starts, four
// workgroups of four wavefronts a compute unit: 4 waves a SIMD.  The second ring could be had in three ways:
//   * a second ring for every group: 72 KiB and more a workgroup at a ring of 128 positions, two workgroups a compute
//     unit, 2 waves a SIMD;
//   * bwd read from the global workspace: the sampler's LDS and every group at work, but an 8-byte global load per
//     candidate in the forward pass, on the word's critical path;
//   * HALF THE GROUPS whenever both rings of all 32 groups do not fit the 32 KiB.  Taken: a ring of up to 64 positions
//     (keys of at most 63 bytes, which is every vocabulary in use) keeps all 32 groups; only vocabularies with longer
//     keys pay, with 16, 8 or 4 groups at work.
// AS BUILT the kernel runs at 3 waves a SIMD whichever way: it takes 137 VGPRs (3 waves), and its LDS is 14 KiB of word
// starts, table and sums plus the rings -- 22 KiB at a ring of 16, 30 KiB at 32 (5 workgroups a compute unit), 46 KiB from
// a ring of 64 on (3 workgroups).  So the registers and, from a ring of 64 on, the LDS both stand at 3, and occupancy no
// longer separates the third option from the second as it was meant to: what is left in its favour is that the forward
// pass reads bwd from LDS.  Getting back to 4 waves needs both fewer registers and the table or the word starts out of LDS.
//
// ACCUMULATION.  A handful of pieces receive a large share of all posteriors from every compute unit.  Two forms, by a
// flag of the entry point: plain f64 atomics into expected[V] from every lane, or a table of ACC_SLOTS (id, f64 sum) in
// LDS per workgroup, direct-mapped by the id's low bits: the first id to reach a slot owns it for the chunk, another id
// that maps there goes to the global array at once, and the table is flushed by global atomics at the chunk's end.  Both
// atomics are the hardware's (ds_add_f64, global_atomic_add_f64: unsafeAtomicAdd, the arrays are ordinary device memory).
#pragma once

namespace {

constexpr int ACC_SLOTS = 512;  // 6 KiB of LDS
constexpr uint32_t EST_PLAIN_ATOMICS = 1u;  // HUTK_UG_ESTEP_PLAIN_ATOMICS

struct EstepArgs {
    const double* low;  // the lowest score alive
    double* beta;       // [cap + 1]: bwd of the words that do not fit their group's ring
    double* expected;   // [n_pieces], added to
    double* stats;      // [2], added to: the sum of Z, the words
};

// sample_trip for the training kernels: a dead piece (its score is NaN) is no candidate, and the unknown edge stands where
// no ALIVE key is the single character.  *x: the candidate's score.
__device__ __forceinline__ int32_t train_trip(const U::Vocab& V, double unk_score, const uint8_t* w, int64_t s, int64_t n, int base,
                                              uint64_t lens, int top, int m, uint32_t& state, int gl, int g0, double* x) {
    const int idx = base + gl, len = idx + 1;
    const uint32_t mine = s + idx < n ? w[s + idx] : 0u;
    uint32_t h = state;
#pragma unroll
    for (int j = 0; j < GROUP; j++) {
        const uint32_t bj = __shfl(mine, g0 + j);
        if (j <= gl) h = U::hash_step(h, bj);
    }
    state = __shfl(h, g0 + GROUP - 1);
    int32_t id = -1;
    if (s + len <= n && len <= top && U::has_len(lens, len)) id = U::find(V, U::hash_end(h), w + s, len);
    double score = id >= 0 ? V.scores[id] : 0.0;
    if (score != score) id = -1;
    if (base == 0) {
        const bool single = group_ballot(id >= 0 && len == m, g0) != 0;
        if (!single && len == m) id = V.unk, score = unk_score;
    }
    *x = score;
    return id;
}

template <bool TABLE>
__device__ __forceinline__ void acc_add(double* expected, int32_t* s_id, double* s_sum, int32_t id, double v) {
    if constexpr (TABLE) {
        const int slot = id & (ACC_SLOTS - 1);
        const int32_t old = atomicCAS(&s_id[slot], -1, id);
        if (old == -1 || old == id) {
            unsafeAtomicAdd(&s_sum[slot], v);
            return;
        }
    }
    unsafeAtomicAdd(&expected[id], v);
}

// The word that starts at ws, by the GROUP lanes of one group (as sample_word).  rb: the group's ring of bwd, as the
// sampler's; rf: its ring of fwd, -inf wherever a position holds nothing, all -inf between words.  z, words: lane 0's sums.
template <bool TABLE>
__device__ __forceinline__ void estep_word(const MatchArgs& a, const EstepArgs& ea, const U::Text& f, int64_t ws, double* rb, double* rf,
                                           int gl, int g0, int32_t* s_id, double* s_sum, double& z, double& words) {
    const int R1 = a.ring - 1;
    const uint8_t* w = f.bytes + ws;
    const double unk_score = *ea.low - 10.0;
    int64_t n = 0;  // the word's bytes
    for (int64_t base = 1; n == 0; base += GROUP) {
        const uint32_t em = group_ballot(U::word_ends(f, ws + base + gl), g0);
        if (em) n = base + __ffs(em) - 1;
    }
    const bool in_lds = n < a.ring;
    group_sync();  // (the forward pass of the group's last word has read the ring)
    if (gl == 0) rb[(int)(n & R1)] = 0.0;

    // bwd[s] = log sum exp(x + bwd[e]), the starts in falling order: k_ug_sample's filter
    for (int64_t hi = n - 1; hi >= 0; hi -= GROUP) {
        const int64_t p = hi - gl;
        for (uint32_t sm = group_ballot(p >= 0 && char_starts(w, p, n), g0); sm; sm &= sm - 1) {
            const int64_t s = hi - (__ffs(sm) - 1);
            group_sync();
            const uint64_t lens = a.V.lens[w[s]];
            const int top = U::top_len(lens, a.V.max_len);
            const int m = U::char_len(w, s, n);
            double mx = -INFINITY, sum = 0.0;
            uint32_t state = U::HASH_INIT;
            for (int base = 0; base == 0 || (base < top && s + base < n); base += GROUP) {
                double x;
                if (train_trip(a.V, unk_score, w, s, n, base, lens, top, m, state, gl, g0, &x) < 0) continue;
                x += rb[(int)((s + base + gl + 1) & R1)];
                if (x > mx) {
                    sum = sum * exp(mx - x) + 1.0;
                    mx = x;
                } else {
                    sum += exp(x - mx);
                }
            }
            double top_x = mx;
#pragma unroll
            for (int d = 1; d < GROUP; d <<= 1) top_x = fmax(top_x, __shfl_xor(top_x, d));
            double total = sum * exp(mx - top_x);
#pragma unroll
            for (int d = 1; d < GROUP; d <<= 1) total += __shfl_xor(total, d);
            if (gl == 0) {
                const double b = top_x + log(total);
                rb[(int)(s & R1)] = b;
                if (!in_lds) ea.beta[ws + s] = b;
            }
        }
    }
    if (!in_lds) __threadfence_block();  // lane 0's stores, for the group's other lanes
    group_sync();
    const double Z = in_lds ? rb[0] : ea.beta[ws];

    // fwd[e] = log sum exp(fwd[s] + x), the starts in rising order; a start's candidates end at distinct positions, a lane each
    if (gl == 0) rf[0] = 0.0;
    for (int64_t s = 0; s < n;) {
        group_sync();
        const double fs = rf[(int)(s & R1)];
        group_sync();
        if (gl == 0) rf[(int)(s & R1)] = -INFINITY;  // (the slot is position s + R's next)
        const uint64_t lens = a.V.lens[w[s]];
        const int top = U::top_len(lens, a.V.max_len);
        const int m = U::char_len(w, s, n);
        uint32_t state = U::HASH_INIT;
        for (int base = 0; base == 0 || (base < top && s + base < n); base += GROUP) {
            double x;
            const int32_t id = train_trip(a.V, unk_score, w, s, n, base, lens, top, m, state, gl, g0, &x);
            if (id < 0) continue;
            const int64_t e = s + base + gl + 1;  // (byte ws + n of the workspace is the next word's first)
            const double b = e >= n ? 0.0 : in_lds ? rb[(int)(e & R1)] : ea.beta[ws + e];
            const double y = fs + x;
            acc_add<TABLE>(ea.expected, s_id, s_sum, id, exp(y + b - Z));
            double* cur = rf + (int)(e & R1);
            const double c = *cur;
            *cur = c == -INFINITY ? y : fmax(c, y) + log1p(exp(-fabs(c - y)));
        }
        s += m;
    }
    group_sync();
    if (gl == 0) {
        rf[(int)(n & R1)] = -INFINITY;
        z += Z;
        words += 1.0;
    }
}

// the sum of v over the workgroup, in thread 0 (s_red: four values of LDS)
__device__ __forceinline__ double block_sum(double v, double* s_red) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double total = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    __syncthreads();
    return total;
}

template <bool TABLE>
__global__ __launch_bounds__(TB) void k_ug_estep(const MatchArgs a, const EstepArgs ea) {
    extern __shared__ double s_ring[];  // [2][n_groups][ring]: bwd, fwd
    __shared__ int s_part[TB / 64];
    __shared__ int s_next;
    __shared__ uint16_t s_ws[U::CHUNK_BYTES];
    __shared__ double s_red[TB / 64];
    __shared__ double s_sum[TABLE ? ACC_SLOTS : 1];
    __shared__ int32_t s_id[TABLE ? ACC_SLOTS : 1];
    if (!*a.ok) return;
    U::Text f = a.f;
    f.n = *a.n_dev;
    const int64_t c0 = (int64_t)blockIdx.x * U::CHUNK_BYTES;
    if (c0 >= f.n) return;
    const int tid = threadIdx.x;
    const int n_words = list_words(f, c0, s_part, s_ws);
    for (int i = tid; i < a.n_groups * a.ring; i += TB) s_ring[a.n_groups * a.ring + i] = -INFINITY;
    if constexpr (TABLE)
        for (int i = tid; i < ACC_SLOTS; i += TB) s_id[i] = -1, s_sum[i] = 0.0;
    if (tid == 0) s_next = 0;
    __syncthreads();
    const int gl = tid & (GROUP - 1), g0 = (tid & 63) & ~(GROUP - 1), g = tid / GROUP;
    double z = 0.0, words = 0.0;
    if (g < a.n_groups) {
        for (;;) {
            int i = 0;
            if (gl == 0) i = atomicAdd(&s_next, 1);
            i = __shfl(i, g0);
            if (i >= n_words) break;
            estep_word<TABLE>(a, ea, f, c0 + s_ws[i], s_ring + g * a.ring, s_ring + (a.n_groups + g) * a.ring, gl, g0, s_id, s_sum, z, words);
        }
    }
    z = block_sum(z, s_red);  // (its barriers stand behind every group's last word: the table is whole)
    words = block_sum(words, s_red);
    if (tid == 0 && words > 0.0) {
        unsafeAtomicAdd(&ea.stats[0], z);
        unsafeAtomicAdd(&ea.stats[1], words);
    }
    if constexpr (TABLE)
        for (int i = tid; i < ACC_SLOTS; i += TB)
            if (s_id[i] >= 0) unsafeAtomicAdd(&ea.expected[s_id[i]], s_sum[i]);
}

__global__ __launch_bounds__(TB) void k_ug_lattice_train(const MatchArgs a, const TrainArgs t) {
    extern __shared__ double s_ring[];  // [n_groups][ring]
    __shared__ int s_part[TB / 64];
    __shared__ int s_next;
    __shared__ uint16_t s_ws[U::CHUNK_BYTES];
    if (!*a.ok) return;
    U::Text f = a.f;
    f.n = *a.n_dev;
    const int64_t c0 = (int64_t)blockIdx.x * U::CHUNK_BYTES;
    if (c0 >= f.n) return;
    const int tid = threadIdx.x;
    const int n_words = list_words(f, c0, s_part, s_ws);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int i = tid; i < a.n_groups * a.ring; i += TB) s_ring[i] = nan;
    if (tid == 0) s_next = 0;
    __syncthreads();
    const int gl = tid & (GROUP - 1), g0 = (tid & 63) & ~(GROUP - 1), g = tid / GROUP;
    if (g >= a.n_groups) return;
    for (;;) {
        int i = 0;
        if (gl == 0) i = atomicAdd(&s_next, 1);
        i = __shfl(i, g0);
        if (i >= n_words) break;
        lattice_word<true>(a, t, f, c0 + s_ws[i], s_ring + g * a.ring, gl, g0);
    }
}

// freq[id] += the times id stands in the id workspace: the table of k_ug_estep with counts of 32 bits (a chunk holds at most
// CHUNK_BYTES ids)
__global__ __launch_bounds__(TB) void k_ug_hist(const MatchArgs a, unsigned long long* freq) {
    __shared__ int32_t s_id[ACC_SLOTS];
    __shared__ uint32_t s_cnt[ACC_SLOTS];
    if (!*a.ok) return;
    const int64_t n = *a.n_dev, c0 = (int64_t)blockIdx.x * U::CHUNK_BYTES;
    if (c0 >= n) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < ACC_SLOTS; i += TB) s_id[i] = -1, s_cnt[i] = 0;
    __syncthreads();
    const int64_t at = c0 + (int64_t)tid * U::SLICE_BYTES;
    for (int64_t p = at; p < at + U::SLICE_BYTES && p < n; p++) {
        const int32_t v = a.tmp[p];
        if (v < 0) continue;
        const int32_t id = v & U::ID_MASK;
        const int slot = id & (ACC_SLOTS - 1);
        const int32_t old = atomicCAS(&s_id[slot], -1, id);
        if (old == -1 || old == id) atomicAdd(&s_cnt[slot], 1u);
        else atomicAdd(&freq[id], 1ull);
    }
    __syncthreads();
    for (int i = tid; i < ACC_SLOTS; i += TB)
        if (s_id[i] >= 0) atomicAdd(&freq[s_id[i]], (unsigned long long)s_cnt[i]);
}

// ---- the M-step ----
// `tokenizers`' digamma: the recurrence up to 7, then the asymptotic series
__device__ __forceinline__ double ug_digamma(double x) {
    double r = 0.0;
    while (x < 7.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    x -= 0.5;
    const double xx = 1.0 / x, xx2 = xx * xx, xx4 = xx2 * xx2;
    return r + log(x) + (1.0 / 24.0) * xx2 - (7.0 / 960.0) * xx4 + (31.0 / 8064.0) * xx4 * xx2 - (127.0 / 30720.0) * xx4 * xx4;
}

struct MstepArgs {
    const double* expected;  // [n]
    double* scores;          // [n], written
    double* scores_out;      // [n] or NULL: a copy for the caller
    int64_t n;
    int32_t unk;
    double* acc;             // [0] the survivors' sum, [1] the lowest score alive
    int64_t* alive;          // [1]
};

__global__ void k_ug_mstep_init(double* acc, int64_t* alive) {
    acc[0] = 0.0;
    acc[1] = INFINITY;
    *alive = 0;
}

__global__ __launch_bounds__(TB) void k_ug_mstep_sum(const MstepArgs a) {
    __shared__ double s_red[TB / 64];
    double mine = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * TB) {
        const double c = a.expected[i];
        if (i != a.unk && c >= 0.5) mine += c;
    }
    const double total = block_sum(mine, s_red);
    if (threadIdx.x == 0 && total > 0.0) unsafeAtomicAdd(&a.acc[0], total);
}

__global__ __launch_bounds__(TB) void k_ug_mstep_score(const MstepArgs a) {
    __shared__ double s_low[TB / 64];
    __shared__ double s_red[TB / 64];
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double of_sum = ug_digamma(a.acc[0]);
    double low = INFINITY, n_alive = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * TB) {
        const double c = a.expected[i];
        double sc = nan;
        if (i != a.unk && c >= 0.5) {
            sc = ug_digamma(c) - of_sum;
            low = fmin(low, sc);
            n_alive += 1.0;
        }
        a.scores[i] = sc;
        if (a.scores_out) a.scores_out[i] = sc;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) low = fmin(low, __shfl_xor(low, d));
    if ((threadIdx.x & 63) == 0) s_low[threadIdx.x >> 6] = low;
    const double total = block_sum(n_alive, s_red);
    if (threadIdx.x == 0) {
        low = fmin(fmin(s_low[0], s_low[1]), fmin(s_low[2], s_low[3]));
        if (total > 0.0) {
            atomicAdd((unsigned long long*)a.alive, (unsigned long long)total);
            unsigned long long* at = (unsigned long long*)&a.acc[1];  // the minimum, by compare and swap
            unsigned long long seen = *at;
            while (low < __longlong_as_double((long long)seen)) {
                const unsigned long long was = atomicCAS(at, seen, (unsigned long long)__double_as_longlong(low));
                if (was == seen) break;
                seen = was;
            }
        }
    }
}

// ---- the prune ----
enum : int32_t { CLS_DEAD = 0, CLS_KEEP = 1, CLS_DROP = 2, CLS_ALT = 3 };

// the key blob as a text: a flag at every key's first byte, and its size where the kernels read the folded text's
__global__ __launch_bounds__(TB) void k_ug_key_flags(const U::Vocab V, int64_t n_slots, uint8_t* flag, int64_t* n_dev, int64_t n_keys) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i == 0) *n_dev = n_keys;
    if (i < n_slots && V.slots[i].id >= 0) flag[V.slots[i].key] = 1;
}

__global__ __launch_bounds__(TB) void k_ug_fill_i32(int32_t* v, int64_t n, int32_t x) {
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) v[i] = x;
}
__global__ __launch_bounds__(TB) void k_ug_fill_f64(double* v, int64_t n, double x) {
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) v[i] = x;
}

// a lane a slot: fin[key] is the score of the key's best path without its spanning edge
__global__ __launch_bounds__(TB) void k_ug_alt_class(const U::Vocab V, int64_t n_slots, const double* fin, int32_t* cls, int32_t* cls_out,
                                                     int64_t* key_at) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n_slots) return;
    const U::Slot e = V.slots[i];
    if (e.id < 0) return;
    const double sc = V.scores[e.id], other = fin[e.key];
    const int32_t c = sc != sc ? CLS_DEAD : other != other ? CLS_KEEP : other > sc ? CLS_DROP : CLS_ALT;
    cls[e.id] = c;
    if (cls_out) cls_out[e.id] = c;
    if (key_at) key_at[e.id] = e.key;
}

__global__ __launch_bounds__(1024) void k_ug_vsum(const int64_t* freq, int64_t n, int64_t* out) {
    __shared__ int64_t s_part[16];
    int64_t mine = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) mine += freq[i];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) mine += __shfl_xor(mine, d);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t total = 0;
        for (int u = 0; u < 16; u++) total += s_part[u];
        *out = total;
    }
}

// a lane a slot: +inf for a piece that is kept whatever it costs, -inf for one that is dropped, else the loss
__global__ __launch_bounds__(TB) void k_ug_loss(const U::Vocab V, int64_t n_slots, const int32_t* cls, const int32_t* alt,
                                                const int64_t* freq, const int64_t* vsum_at, double* loss) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n_slots) return;
    const U::Slot e = V.slots[i];
    if (e.id < 0) return;
    const int32_t c = cls[e.id];
    if (c == CLS_DEAD) return;
    const double fi = (double)freq[e.id], vsum = (double)*vsum_at;
    double out;
    if (c == CLS_KEEP) {
        out = INFINITY;
    } else if (c == CLS_DROP || fi == 0.0) {
        out = -INFINITY;
    } else {
        int n_alt = 0;
        for (uint32_t p = 0; p < e.len; p++) n_alt += alt[e.key + p] >= 0;
        const double of_all = log(vsum + fi * (double)(n_alt - 1));
        double lp_alt = 0.0;
        for (uint32_t p = 0; p < e.len; p++) {
            const int32_t v = alt[e.key + p];
            if (v >= 0) lp_alt += log((double)freq[v & U::ID_MASK] + fi) - of_all;
        }
        out = fi / vsum * (log(fi) - log(vsum) - lp_alt);
    }
    loss[e.id] = out;
}

__global__ void k_ug_low_init(double* acc, double low) {
    acc[0] = 0.0;
    acc[1] = low;
}

// What every training entry starts with (the caller holds h->mu): the handle's device, and once per handle the scalars of
// training on it -- [0] the M-step's sum, [1] the lowest score alive --, written by a kernel on the caller's stream (the
// allocation may wait once, like every growth of the workspace).
int ug_train_ready(hutk_unigram* h, hipStream_t st) {
    HUTK_HIP_TRY(hipSetDevice(h->device));
    if (h->train_ready) return HUTK_OK;
    HUTK_HIP_TRY(h->t_low.reserve(2));
    hipLaunchKernelGGL(k_ug_low_init, dim3(1), dim3(1), 0, st, h->t_low.p, h->V.unk_score + 10.0);
    HUTK_HIP_TRY(hipGetLastError());
    h->train_ready = true;
    return HUTK_OK;
}

size_t train_rings(const hutk_unigram* h, int32_t& n_groups) {
    n_groups = std::min(GROUPS, RING_LDS_BYTES / (16 * h->ring));
    return 2 * (size_t)n_groups * h->ring * sizeof(double);
}

}  // namespace

extern "C" {

int64_t hutk_unigram_key_bytes(const hutk_unigram* h) { return h ? h->n_key_bytes : -1; }

int hutk_unigram_set_scores(hutk_unigram* h, const double* scores, void* hip_stream) {
    if (!h || !scores) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_set_scores: bad arguments");
    std::vector<double> v(scores, scores + h->n_pieces);
    const double nan = std::nan("");
    v[(size_t)h->unk] = nan;
    double low = INFINITY;
    for (double x : v) {
        if (std::isinf(x)) return hutk::api_set_error(HUTK_E_VALUE, "hutk_unigram_set_scores: a score is infinite");
        if (x == x) low = std::min(low, x);
    }
    if (low == INFINITY) return hutk::api_set_error(HUTK_E_VALUE, "hutk_unigram_set_scores: no piece is alive");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = ug_train_ready(h, st)) return rc;
    if (h->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
    HUTK_HIP_TRY(hipMemcpyAsync(h->d_scores.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HUTK_HIP_TRY(hipMemcpyAsync(h->t_low.p + 1, &low, sizeof(double), hipMemcpyHostToDevice, st));
    HUTK_HIP_TRY(hipStreamSynchronize(st));  // (the sources are this call's own)
    return ug_back(h, st);
}

int hutk_unigram_estep_device(hutk_unigram* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                              double* d_expected, double* d_stats, uint32_t flags, int32_t* d_err, void* hip_stream) {
    const std::string who = "hutk_unigram_estep_device";
    if (!h) return hutk::api_set_error(HUTK_E_ARG, who + ": the handle is NULL");
    if (n_docs < 0 || n_bytes < 0 || !d_offsets || !d_expected || !d_stats || (n_bytes > 0 && !d_bytes) || (flags & ~EST_PLAIN_ATOMICS))
        return hutk::api_set_error(HUTK_E_ARG, who + ": bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = ug_train_ready(h, st)) return rc;
    MatchArgs m;
    int64_t chunks = 0;
    if (int rc = ug_front(h, d_bytes, d_offsets, n_docs, n_bytes, false, d_err, st, who, m, chunks)) return rc;
    if (chunks) {
        const size_t rings = train_rings(h, m.n_groups);
        const EstepArgs ea{h->t_low.p + 1, reinterpret_cast<double*>(h->w_bp.p), d_expected, d_stats};
        if (flags & EST_PLAIN_ATOMICS) hipLaunchKernelGGL(k_ug_estep<false>, dim3((unsigned)chunks), dim3(TB), rings, st, m, ea);
        else hipLaunchKernelGGL(k_ug_estep<true>, dim3((unsigned)chunks), dim3(TB), rings, st, m, ea);
    }
    return ug_back(h, st);
}

int hutk_unigram_mstep_device(hutk_unigram* h, const double* d_expected, double* d_scores_out, int64_t* d_alive, void* hip_stream) {
    if (!h || !d_expected || !d_alive) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_mstep_device: bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = ug_train_ready(h, st)) return rc;
    if (h->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
    const MstepArgs a{d_expected, h->d_scores.p, d_scores_out, h->n_pieces, h->unk, h->t_low.p, d_alive};
    const unsigned blocks = (unsigned)std::min<int64_t>((h->n_pieces + TB - 1) / TB, 1024);
    hipLaunchKernelGGL(k_ug_mstep_init, dim3(1), dim3(1), 0, st, a.acc, a.alive);
    hipLaunchKernelGGL(k_ug_mstep_sum, dim3(blocks), dim3(TB), 0, st, a);
    hipLaunchKernelGGL(k_ug_mstep_score, dim3(blocks), dim3(TB), 0, st, a);
    return ug_back(h, st);
}

int hutk_unigram_alternatives_device(hutk_unigram* h, int32_t* d_class, int32_t* d_path, int64_t* d_key_at, void* hip_stream) {
    if (!h) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_alternatives_device: the handle is NULL");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = ug_train_ready(h, st)) return rc;
    const int64_t nk = h->n_key_bytes, chunks = (nk + U::CHUNK_BYTES - 1) / U::CHUNK_BYTES;
    HUTK_HIP_TRY(h->t_kflag.reserve((size_t)nk + 1));
    HUTK_HIP_TRY(h->t_alt.reserve((size_t)nk + 1));
    HUTK_HIP_TRY(h->t_fin.reserve((size_t)nk + 1));
    HUTK_HIP_TRY(h->t_kbp.reserve((size_t)nk + 1));
    HUTK_HIP_TRY(h->t_class.reserve((size_t)h->n_pieces));
    if (h->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
    int32_t* ok = h->w_ok.p;
    int64_t* n_dev = h->w_small.p + 1;
    HUTK_HIP_TRY(hipMemsetAsync(ok, 1, sizeof(int32_t), st));
    HUTK_HIP_TRY(hipMemsetAsync(h->t_kflag.p, 0, (size_t)nk + 1, st));
    const unsigned slot_blocks = blocks_for(h->n_slots);
    hipLaunchKernelGGL(k_ug_key_flags, dim3(slot_blocks), dim3(TB), 0, st, h->V, h->n_slots, h->t_kflag.p, n_dev, nk);
    const unsigned fill = (unsigned)std::min<int64_t>((std::max(nk, h->n_pieces) + TB) / TB, 1 << 16);
    hipLaunchKernelGGL(k_ug_fill_i32, dim3(fill), dim3(TB), 0, st, h->t_alt.p, nk, -1);
    hipLaunchKernelGGL(k_ug_fill_i32, dim3(fill), dim3(TB), 0, st, h->t_class.p, h->n_pieces, (int32_t)CLS_DEAD);
    if (d_class) hipLaunchKernelGGL(k_ug_fill_i32, dim3(fill), dim3(TB), 0, st, d_class, h->n_pieces, (int32_t)CLS_DEAD);
    if (d_key_at) HUTK_HIP_TRY(hipMemsetAsync(d_key_at, 0xFF, (size_t)h->n_pieces * sizeof(int64_t), st));  // (-1: the piece has no key)
    MatchArgs m{};
    m.f = U::Text{h->d_keys.p, h->t_kflag.p, nk}, m.n_dev = n_dev, m.V = h->V, m.ring = h->ring, m.n_groups = h->n_groups;
    m.tmp = h->t_alt.p, m.bp = h->t_kbp.p, m.n_chunks = chunks, m.ok = ok;
    const TrainArgs t{h->t_low.p + 1, h->t_fin.p, 1};
    if (chunks)
        hipLaunchKernelGGL(k_ug_lattice_train, dim3((unsigned)chunks), dim3(TB), (size_t)h->n_groups * h->ring * sizeof(double), st, m, t);
    hipLaunchKernelGGL(k_ug_alt_class, dim3(slot_blocks), dim3(TB), 0, st, h->V, h->n_slots, h->t_fin.p, h->t_class.p, d_class, d_key_at);
    if (d_path && nk) HUTK_HIP_TRY(hipMemcpyAsync(d_path, h->t_alt.p, (size_t)nk * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return ug_back(h, st);
}

int hutk_unigram_hist_device(hutk_unigram* h, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n_docs, int64_t n_bytes,
                             int64_t* d_freq, int32_t* d_err, void* hip_stream) {
    const std::string who = "hutk_unigram_hist_device";
    if (!h) return hutk::api_set_error(HUTK_E_ARG, who + ": the handle is NULL");
    if (n_docs < 0 || n_bytes < 0 || !d_offsets || !d_freq || (n_bytes > 0 && !d_bytes)) return hutk::api_set_error(HUTK_E_ARG, who + ": bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = ug_train_ready(h, st)) return rc;
    MatchArgs m;
    int64_t chunks = 0;
    if (int rc = ug_front(h, d_bytes, d_offsets, n_docs, n_bytes, false, d_err, st, who, m, chunks)) return rc;
    if (chunks) {
        const TrainArgs t{h->t_low.p + 1, nullptr, 0};
        hipLaunchKernelGGL(k_ug_lattice_train, dim3((unsigned)chunks), dim3(TB), (size_t)h->n_groups * h->ring * sizeof(double), st, m, t);
        hipLaunchKernelGGL(k_ug_hist, dim3((unsigned)chunks), dim3(TB), 0, st, m, reinterpret_cast<unsigned long long*>(d_freq));
    }
    return ug_back(h, st);
}

int hutk_unigram_prune_loss_device(hutk_unigram* h, const int64_t* d_freq, double* d_loss, void* hip_stream) {
    if (!h || !d_freq || !d_loss) return hutk::api_set_error(HUTK_E_ARG, "hutk_unigram_prune_loss_device: bad arguments");
    std::lock_guard<std::mutex> lock(h->mu);
    if (!h->t_class.p || !h->t_alt.p)
        return hutk::api_set_error(HUTK_E_VALUE, "hutk_unigram_prune_loss_device: hutk_unigram_alternatives_device has not run on this handle");
    hipStream_t st = (hipStream_t)hip_stream;
    HUTK_HIP_TRY(hipSetDevice(h->device));
    if (h->ev_recorded) HUTK_HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
    int64_t* vsum = h->w_small.p + 2;
    const unsigned fill = (unsigned)std::min<int64_t>((h->n_pieces + TB) / TB, 1 << 16);
    hipLaunchKernelGGL(k_ug_fill_f64, dim3(fill), dim3(TB), 0, st, d_loss, h->n_pieces, std::nan(""));
    hipLaunchKernelGGL(k_ug_vsum, dim3(1), dim3(1024), 0, st, d_freq, h->n_pieces, vsum);
    hipLaunchKernelGGL(k_ug_loss, dim3(blocks_for(h->n_slots)), dim3(TB), 0, st, h->V, h->n_slots, h->t_class.p, h->t_alt.p, d_freq, vsum, d_loss);
    return ug_back(h, st);
}

}  // extern "C"
