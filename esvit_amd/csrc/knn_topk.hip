// esvit_gemm_desc::topk -- the k-nearest-neighbour epilogue of the exact-fp32 GEMM (eval_knn.py:197-210 without the dense
// [rows, N_train] similarity block): similarity and selection in one pass over the train matrix.
//
// Phase 1 (knn_scan_kernel): one workgroup per (128 test rows, train split).  It walks its train range in 128-column tiles on the
// register-staged fp32 main loop of gemm_kernels.h (v_mfma_f32_16x16x4_f32; every similarity is ONE chain over K in k order --
// the same chain wherever the column lies, in whichever call).  After a tile's loop every value is compared with its row's
// threshold tau (LDS; the k-th best so far, -inf before the first compaction).  The accumulator tile goes through LDS so that one
// wave sees whole rows: survivors (value >= tau) are appended in column order to the (row, split) candidate list in the global
// scratch (slots from a ballot prefix over the row's counter -- no atomics, no float order that depends on timing).  A list holds
// CAP = 2 k + 128 entries: a tile adds at most 128 per row, so a list that enters a tile with at most CAP - 128 entries cannot
// overflow; at the tile boundary every list above that mark is compacted to its best k by the total order and tau is raised.
// The set a list holds at a tile boundary, hence tau, hence the next tile's survivors, are the same in every launch.
//
// Phase 2 (knn_merge_kernel): one workgroup per test row gathers the row's split lists (each compacted to <= k at the end of
// phase 1) and, with merge, the list already in vals / idx; selects the k best and writes them sorted.
//
// The total order: larger value first, on equal values the smaller train row number first.  It is carried by one 64-bit key,
// (order-preserving bits of the float) << 32 | ~row number; "best k of n" is the k-th largest key found bit by bit (64 counting
// passes), keys are distinct, so exactly k elements lie at or above it.  -0.0 is stored as +0.0 (equal floats, one key).
#include "gemm_kernels.h"

namespace {

constexpr int KNN_BM = 128, KNN_BN = 128;
constexpr int KNN_MAX_K = 256;
constexpr int KNN_MAX_SPLITS = 28;                                // phase 2 holds splits * k + k keys in LDS (58 KiB at k = 256)
constexpr int KNN_MERGE_KEYS = KNN_MAX_SPLITS * KNN_MAX_K + KNN_MAX_K;
constexpr int KNN_SLOTS = 512;                                    // resident workgroups of phase 1 (two per CU)
constexpr int KNN_STAGE_LD = KNN_BN + 4;                             // the accumulator tile in LDS, 128 x 132 floats inside the operand buffers
constexpr int KNN_NE = (2 * KNN_MAX_K + KNN_BN + 63) / 64;        // keys per lane when one wave holds a whole list

typedef unsigned long long u64;

struct KnnEntry {
    float v;
    int i;
};

struct KnnPlan {
    int row_tiles, col_tiles, tiles_per_split, splits, cap;
    long lists;  // (row tile, split) lists the workspace is sized for
};

// a pure function of (M, N, k): esvit_query and the launch agree by construction
KnnPlan knn_plan(long M, long N, int k) {
    KnnPlan p;
    p.row_tiles = ceil_div(M, KNN_BM);
    p.col_tiles = ceil_div(N, KNN_BN);
    const int by_n = p.col_tiles / 8 > 1 ? p.col_tiles / 8 : 1;  // a split scans at least 8 column tiles
    const int s_cap = by_n < KNN_MAX_SPLITS ? by_n : KNN_MAX_SPLITS;
    int s = KNN_SLOTS / p.row_tiles;  // fill the chip once: whole rounds of equally long workgroups
    if (s < 1) s = 1;
    if (s > s_cap) s = s_cap;
    p.tiles_per_split = ceil_div(p.col_tiles, s);
    p.splits = ceil_div(p.col_tiles, p.tiles_per_split);
    p.cap = 2 * k + KNN_BN;
    // sized by a bound that is monotone in M (row_tiles * splits itself dips where the split count steps down)
    const long full = (long)p.row_tiles * s_cap, flat = p.row_tiles > KNN_SLOTS ? p.row_tiles : KNN_SLOTS;
    p.lists = full < flat ? full : flat;
    return p;
}

long knn_ws_bytes(const KnnPlan& p) { return p.lists * KNN_BM * ((long)p.cap * sizeof(KnnEntry) + sizeof(int)); }

__device__ __forceinline__ unsigned knn_ord(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unord(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
__device__ __forceinline__ u64 knn_key(float v, int i) { return ((u64)knn_ord(v) << 32) | (unsigned)(~i); }

// One wave cuts the list of one row (n <= 64 KNN_NE entries) down to its best k (n > k).  Returns the k-th best value.
// (A call, not inlined: inlined into the scan its registers came on top of the main loop's and the kernel spilled.)
__device__ __noinline__ float knn_compact_row(KnnEntry* __restrict__ list, int n, int k, int lane) {
    u64 key[KNN_NE];
#pragma unroll
    for (int t = 0; t < KNN_NE; ++t) {
        const int s = lane + 64 * t;
        key[t] = 0;  // (below every real key: a finite float's ordered bits are never 0)
        if (s < n) {
            const KnnEntry e = list[s];
            key[t] = knn_key(e.v, e.i);
        }
    }
    u64 T = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const u64 cand = T | (1ull << bit);
        int cnt = 0;
#pragma unroll
        for (int t = 0; t < KNN_NE; ++t) cnt += __popcll(__ballot(key[t] >= cand));
        if (cnt >= k) T = cand;
    }
    // every load of the list is complete (the search consumed it): rewrite the winners in place, slots 0 .. k - 1
    int base = 0;
#pragma unroll
    for (int t = 0; t < KNN_NE; ++t) {
        const bool win = key[t] >= T;
        const u64 m = __ballot(win);
        if (win) {
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            KnnEntry e;
            e.v = knn_unord((unsigned)(key[t] >> 32));
            e.i = (int)~(unsigned)key[t];
            list[pos] = e;
        }
        base += __popcll(m);
    }
    return knn_unord((unsigned)(T >> 32));
}

template <bool WRITE_C>
__global__ __launch_bounds__(NTHREADS, 2) void knn_scan_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ Cmat,
                                                               int M, int N, int K, long lda, long ldb, long ldc, int k, int cap,
                                                               int row_tiles, int tiles_per_split, int col_tiles, int splits,
                                                               KnnEntry* __restrict__ lists, int* __restrict__ counts) {
    using TA = Tile<float, false, KNN_BM, false>;
    using TB = Tile<float, false, KNN_BN, false>;
    constexpr int FM = 4, FN = 4;  // 2 x 2 waves of 64 x 64

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sA = reinterpret_cast<float*>(smem_raw);
    float* sB = sA + 2 * TA::ELEMS;
    float* tau = sB + 2 * TB::ELEMS;
    int* cnt = reinterpret_cast<int*>(tau + KNN_BM);

    const int tm = blockIdx.x % row_tiles, sp = blockIdx.x / row_tiles;
    const int m0 = tm * KNN_BM;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;

    KnnEntry* my_lists = lists + ((long)tm * splits + sp) * KNN_BM * cap;
    if (threadIdx.x < KNN_BM) {
        tau[threadIdx.x] = -INFINITY;
        cnt[threadIdx.x] = 0;
    }

    const int t_beg = sp * tiles_per_split, t_end = min(col_tiles, t_beg + tiles_per_split);
    const int nk = (K + BK - 1) / BK;
    for (int tn = t_beg; tn < t_end; ++tn) {
        const int n0 = tn * KNN_BN;
        f32x4 acc[FM][FN];
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            TA ta;
            TB tb;
            ta.load(A, lda, m0, 0, M, K);
            tb.load(B, ldb, n0, 0, N, K);
            ta.store(sA);
            tb.store(sB);
            __syncthreads();
            for (int kt = 0; kt < nk; ++kt) {
                const int cur = kt & 1;
                if (kt + 1 < nk) {
                    ta.load(A, lda, m0, (kt + 1) * BK, M, K);
                    tb.load(B, ldb, n0, (kt + 1) * BK, N, K);
                }
                const float* a_lds = sA + cur * TA::ELEMS;
                const float* b_lds = sB + cur * TB::ELEMS;
                Frag<float> af[FM], bfr[FN];
#pragma unroll
                for (int i = 0; i < FM; ++i) af[i] = TA::frag(a_lds, wm * 64 + i * 16, c, g);
#pragma unroll
                for (int j = 0; j < FN; ++j) bfr[j] = TB::frag(b_lds, wn * 64 + j * 16, c, g);
                // the k-step outermost: 16 independent accumulators between two MFMAs of one chain (40-clock dependent latency against
                // a 32-clock issue); each accumulator still sees its k-steps in the one fixed order
#pragma unroll
                for (int q = 0; q < 8; ++q)
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int j = 0; j < FN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].v[q], bfr[j].v[q], acc[i][j], 0, 0, 0);
                if (kt + 1 < nk) {
                    ta.store(sA + (cur ^ 1) * TA::ELEMS);
                    tb.store(sB + (cur ^ 1) * TB::ELEMS);
                }
                __syncthreads();
            }
        }
        // acc[i][j][r] = similarity(row m0 + wm 64 + 16 i + 4 g + r, column n0 + wn 64 + 16 j + c): through the (now free) operand LDS,
        // so that one wave sees whole rows -- it appends a row's survivors in column order, and compacts the row when due
        float* stage = reinterpret_cast<float*>(smem_raw);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    stage[(wm * 64 + i * 16 + 4 * g + r) * KNN_STAGE_LD + wn * 64 + j * 16 + c] = acc[i][j][r] + 0.f;  // -0.0 -> +0.0
        __syncthreads();
        const bool last = tn + 1 == t_end;
        const u64 below = (1ull << lane) - 1ull;
        for (int rl = wave; rl < KNN_BM && m0 + rl < M; rl += NTHREADS / 64) {
            const long row = m0 + rl;
            const float th = tau[rl];
            int n = cnt[rl];  // <= cap - 128 on entry, and a tile has 128 columns: the appends stay inside the list
            KnnEntry* list = my_lists + (long)rl * cap;
#pragma unroll
            for (int h = 0; h < KNN_BN / 64; ++h) {
                const int col = n0 + 64 * h + lane;
                const float v = stage[rl * KNN_STAGE_LD + 64 * h + lane];
                const bool in = col < N;
                if constexpr (WRITE_C) {
                    if (in) Cmat[row * ldc + col] = v;
                }
                const bool pass = in && v >= th;
                const u64 m = __ballot(pass);
                if (pass) {
                    KnnEntry e;
                    e.v = v;
                    e.i = col;
                    list[n + __popcll(m & below)] = e;
                }
                n += __popcll(m);
            }
            if (n > k && (last || n > cap - KNN_BN)) {  // tile boundary of this row: cut the list to its best k, raise tau
                __threadfence_block();                 // (the entries other lanes of this wave stored are read back)
                const float t = knn_compact_row(list, n, k, lane);
                n = k;
                if (lane == 0) tau[rl] = t;
            }
            if (lane == 0) cnt[rl] = n;
        }
        __syncthreads();
    }
    if (threadIdx.x < KNN_BM) counts[((long)tm * splits + sp) * KNN_BM + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const KnnEntry* __restrict__ lists, const int* __restrict__ counts, int splits, int cap, int k,
                                                        int merge, long idx_base, float* __restrict__ vals, int* __restrict__ idx) {
    __shared__ u64 keys[KNN_MERGE_KEYS];
    __shared__ u64 win[KNN_MAX_K];
    __shared__ int off[KNN_MAX_SPLITS + 2];
    __shared__ int tally[64];
    __shared__ int nwin;

    const int row = blockIdx.x;
    const int tm = row / KNN_BM, rl = row % KNN_BM;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int n = 0;
        for (int s = 0; s < splits; ++s) {
            off[s] = n;
            n += counts[((long)tm * splits + s) * KNN_BM + rl];  // <= k each: phase 1 ends with a compaction
        }
        off[splits] = n;
        off[splits + 1] = n + (merge ? k : 0);
        nwin = 0;
    }
    if (tid < 64) tally[tid] = 0;
    __syncthreads();
    const int n_scan = off[splits], n = off[splits + 1];
    for (int s = 0; s < splits; ++s) {
        const KnnEntry* list = lists + (((long)tm * splits + s) * KNN_BM + rl) * cap;
        const int b = off[s], cn = off[s + 1] - b;
        for (int t = tid; t < cn; t += 256) {
            const KnnEntry e = list[t];
            keys[b + t] = knn_key(e.v, (int)(e.i + idx_base));
        }
    }
    if (merge)
        for (int t = tid; t < k; t += 256) keys[n_scan + t] = knn_key(vals[(long)row * k + t] + 0.f, idx[(long)row * k + t]);
    __syncthreads();

    // the k-th largest key, bit by bit; one counter per bit, so one barrier per pass
    u64 T = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const u64 cand = T | (1ull << bit);
        int cn = 0;
        for (int t = tid; t < n; t += 256) cn += keys[t] >= cand;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cn += __shfl_xor(cn, o, 64);
        if ((tid & 63) == 0 && cn) atomicAdd(&tally[bit], cn);
        __syncthreads();
        if (tally[bit] >= k) T = cand;
    }
    for (int t = tid; t < n; t += 256) {
        const u64 key = keys[t];
        if (key >= T) {  // exactly k of them while the keys are distinct (the guard: a caller's overlapping idx_base)
            const int pos = atomicAdd(&nwin, 1);
            if (pos < k) win[pos] = key;
        }
    }
    __syncthreads();
    if (tid < k) {
        const u64 mine = win[tid];
        int rank = 0;
        for (int t = 0; t < k; ++t) rank += win[t] > mine;
        vals[(long)row * k + rank] = knn_unord((unsigned)(mine >> 32));
        idx[(long)row * k + rank] = (int)~(unsigned)mine;
    }
}

}  // namespace

int64_t esvit_i_topk_ws(int64_t M, int64_t N, int64_t k) {
    if (M <= 0 || N <= 0 || k < 1 || k > KNN_MAX_K || M > 0x7fffffffL || N > 0x7fffffffL) {
        esvit_set_error("esvit_query(ESVIT_Q_TOPK_WS): needs M > 0, N > 0 and 1 <= k <= %d (M=%ld N=%ld k=%ld)", KNN_MAX_K, (long)M, (long)N, (long)k);
        return ESVIT_ERR_ARG;
    }
    return knn_ws_bytes(knn_plan(M, N, (int)k));
}

void esvit_knn_topk_tile(int* bm, int* bn, int* slots) {
    if (bm) *bm = KNN_BM;
    if (bn) *bn = KNN_BN;
    if (slots) *slots = KNN_SLOTS;
}

// every argument check comes before the first HIP call (a GPU-less host can exercise them); esvit_gemm_select asks without buffers
int esvit_knn_topk_check(int dtype, const esvit_gemm_desc& d, bool with_buffers) {
    const esvit_gemm_topk& t = *d.topk;
    ESVIT_CHECK_ARG(dtype == ESVIT_F32, "esvit_gemm(topk): the k-NN epilogue is exact fp32 only (dtype %d)", dtype);
    ESVIT_CHECK_ARG(t.k >= 1 && t.k <= KNN_MAX_K, "esvit_gemm(topk): k=%d outside 1 .. %d", t.k, KNN_MAX_K);
    ESVIT_CHECK_ARG(d.M > 0 && d.N > 0 && d.K > 0, "esvit_gemm(topk): bad shape M=%d N=%d K=%d", d.M, d.N, d.K);
    ESVIT_CHECK_ARG(t.merge == 0 || t.merge == 1, "esvit_gemm(topk): merge is 0 or 1");
    ESVIT_CHECK_ARG(t.merge || t.k <= d.N, "esvit_gemm(topk): k=%d exceeds the %d train rows and there is no list to merge", t.k, d.N);
    ESVIT_CHECK_ARG(d.K % 4 == 0 && d.lda % 4 == 0 && d.ldb % 4 == 0, "esvit_gemm(topk): K, lda and ldb must be multiples of 4");
    ESVIT_CHECK_ARG(!d.a_kstrided && !d.b_kstrided && d.batch <= 1 && d.splitk <= 1 && !d.partial,
                    "esvit_gemm(topk): row-major operands, one batch, no split-K");
    ESVIT_CHECK_ARG(!d.bias && !d.residual && !d.rowmap && !d.rowscale && !d.aux && d.epilogue == 0 && !d.colsum && !d.colsum_partial && !d.rowstat &&
                        !d.colstat && !d.accumulate,
                    "esvit_gemm(topk): no other epilogue combines with the k-NN selection");
    ESVIT_CHECK_ARG(d.alpha == 1.f, "esvit_gemm(topk): alpha must be 1");
    ESVIT_CHECK_ARG(d.kernel == ESVIT_GEMM_AUTO || d.kernel == ESVIT_GEMM_REGSTAGE, "esvit_gemm(topk): runs on the register-staged fp32 loop only");
    if (!with_buffers) return ESVIT_OK;
    ESVIT_CHECK_ARG(d.A && d.B && t.vals && t.idx && t.workspace, "esvit_gemm(topk): null operand");
    ESVIT_CHECK_ARG(((uintptr_t)d.A % 16 == 0) && ((uintptr_t)d.B % 16 == 0) && ((uintptr_t)t.workspace % 16 == 0), "esvit_gemm(topk): operands and workspace must be 16-byte aligned");
    ESVIT_CHECK_ARG(!d.C || d.ldc >= d.N, "esvit_gemm(topk): ldc=%ld below N=%d", (long)d.ldc, d.N);
    ESVIT_CHECK_ARG(t.idx_base >= 0 && t.idx_base + (int64_t)d.N <= 0x7fffffffL, "esvit_gemm(topk): idx_base + N must fit int32");
    const int64_t need = knn_ws_bytes(knn_plan(d.M, d.N, t.k));
    ESVIT_CHECK_ARG(t.workspace_bytes >= need, "esvit_gemm(topk): workspace of %ld bytes, esvit_query(ESVIT_Q_TOPK_WS) asks for %ld", (long)t.workspace_bytes, (long)need);
    return ESVIT_OK;
}

int esvit_knn_topk_launch(int dtype, const esvit_gemm_desc& d, hipStream_t stream) {
    const int rc = esvit_knn_topk_check(dtype, d, true);
    if (rc != ESVIT_OK) return rc;
    const esvit_gemm_topk& t = *d.topk;
    const KnnPlan p = knn_plan(d.M, d.N, t.k);
    KnnEntry* lists = reinterpret_cast<KnnEntry*>(t.workspace);
    int* counts = reinterpret_cast<int*>(lists + p.lists * KNN_BM * p.cap);
    using TA = Tile<float, false, KNN_BM, false>;
    using TB = Tile<float, false, KNN_BN, false>;
    const size_t lds = 2 * (size_t)(TA::ELEMS + TB::ELEMS) * sizeof(float) + KNN_BM * (sizeof(float) + sizeof(int));
    const dim3 grid(p.row_tiles * p.splits);
    const float* A = reinterpret_cast<const float*>(d.A);
    const float* B = reinterpret_cast<const float*>(d.B);
    if (d.C) {
        auto kern = knn_scan_kernel<true>;
        static unsigned long long lds_set = 0;
        esvit_raise_lds(kern, (int)lds, lds_set);
        hipLaunchKernelGGL(kern, grid, dim3(NTHREADS), lds, stream, A, B, reinterpret_cast<float*>(d.C), d.M, d.N, d.K, (long)d.lda, (long)d.ldb, (long)d.ldc,
                           t.k, p.cap, p.row_tiles, p.tiles_per_split, p.col_tiles, p.splits, lists, counts);
    } else {
        auto kern = knn_scan_kernel<false>;
        static unsigned long long lds_set = 0;
        esvit_raise_lds(kern, (int)lds, lds_set);
        hipLaunchKernelGGL(kern, grid, dim3(NTHREADS), lds, stream, A, B, (float*)nullptr, d.M, d.N, d.K, (long)d.lda, (long)d.ldb, (long)d.ldc, t.k, p.cap,
                           p.row_tiles, p.tiles_per_split, p.col_tiles, p.splits, lists, counts);
    }
    ESVIT_CHECK_LAUNCH("esvit_gemm(topk scan)");
    hipLaunchKernelGGL(knn_merge_kernel, dim3(d.M), dim3(256), 0, stream, lists, counts, p.splits, p.cap, t.k, t.merge, (long)t.idx_base, t.vals, t.idx);
    ESVIT_CHECK_LAUNCH("esvit_gemm(topk merge)");
    return ESVIT_OK;
}
