// cpm_budget.hip -- the budgeted finish of a changed-photon selection: of the photons a selection's tiles list, the `budget` most
// important ones (smallest key, ties by index), chosen on the device by a radix SELECT over the 31 key bits -- digit histograms
// over the listed photons only, no sort, no host read -- and written as an ascending index list for cpm_trace_selected /
// cpm_splat_delta.  Replaces sortIndicesByImportance + the host's min(count, budget) + the keys-only sort of the batch
// (ref processor/progressivephotontracercl.cpp:358-419,467-473).
#include "cpm_selection.h"

#include <chrono>

using namespace cpm;

namespace {

constexpr uint32_t kUnchanged = 2147483647u;
constexpr uint32_t kBins1 = 2048, kBins2 = 1024, kBins3 = 1024;  // key bits 30..20, 19..10, 9..0
static_assert(kBins1 + kBins2 + kBins3 == kBudgetHistWords, "histogram table");

struct BudgetArgs {
    const uint2* tile;      // per tile: (count, start of its list in `local`)
    uint32_t n_tiles;
    const uint32_t* local;  // tile-local lists, ascending
    const uint32_t* keys;   // importance keys, at the photons' own indices
    uint32_t budget;
    uint32_t* hist;         // kBudgetHistWords, zero before the first histogram launch
    uint2* group;           // per workgroup (= kCompactGroup tiles): listed photons with key < T, with key == T
};

// LDS every kernel here shares the shape of
struct BudgetShared {
    uint32_t red[4];
    uint32_t res[2];
    uint2 tiles[kCompactGroup];
    uint32_t off[kCompactGroup + 1];
};

// sum over the workgroup's 256 threads, to all of them
__device__ inline uint32_t block_sum(uint32_t v, BudgetShared& sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();  // (sh.red may still be read from the call before)
    if ((threadIdx.x & 63u) == 0) sh.red[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh.red[0] + sh.red[1] + sh.red[2] + sh.red[3];
}

// |C|: the photons the selection's tiles list
__device__ inline uint32_t listed_total(const BudgetArgs& A, BudgetShared& sh) {
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < A.n_tiles; i += 256u) c += A.tile[i].x;
    return block_sum(c, sh);
}

// The digit in which the `want`-th smallest (1-based) of the keys counted in hist[0 .. bins) lies, and its rank among the keys of
// that digit: the smallest d with hist[0] + .. + hist[d] >= want, rem = want - (hist[0] + .. + hist[d - 1]) in 1 .. hist[d].
// Every workgroup derives it from the small table itself (bins / 256 loads per thread) instead of a scan launch writing it.
__device__ inline void find_digit(const uint32_t* __restrict__ hist, uint32_t bins, uint32_t want, BudgetShared& sh, uint32_t* digit, uint32_t* rem) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, per = bins / 256u;
    uint32_t h[8], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) { h[k] = k < per ? hist[t * per + k] : 0u; sum += h[k]; }
    uint32_t incl = sum;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); incl += (int)lane >= off ? o : 0u; }
    __syncthreads();
    if (lane == 63u) sh.red[wave] = incl;
    if (t == 0) { sh.res[0] = bins - 1u; sh.res[1] = 0u; }  // (a table that does not hold `want` keys: nothing is admitted on the cut)
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) incl += sh.red[w];
    uint32_t excl = incl - sum;
    if (excl < want && want <= incl) {
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            if (k < per && excl < want && want <= excl + h[k]) { sh.res[0] = t * per + k; sh.res[1] = want - excl; }
            excl += h[k];
        }
    }
    __syncthreads();
    *digit = sh.res[0];
    *rem = sh.res[1];
}

// The cut after `levels` digits: the key prefix of the budget-th smallest listed key and how many keys equal to it (in those
// digits) are still to be admitted.  levels == 3: T = the threshold key, r = ties admitted.
__device__ inline void derive_cut(const BudgetArgs& A, int levels, BudgetShared& sh, uint32_t* prefix, uint32_t* rem) {
    uint32_t d = 0, r = A.budget, p = 0;
    if (levels >= 1) { find_digit(A.hist, kBins1, r, sh, &d, &r); p = d; }
    if (levels >= 2) { find_digit(A.hist + kBins1, kBins2, r, sh, &d, &r); p = (p << 10) | d; }
    if (levels >= 3) { find_digit(A.hist + kBins1 + kBins2, kBins3, r, sh, &d, &r); p = (p << 10) | d; }
    *prefix = p;
    *rem = r;
}

// this workgroup's tiles and where their lists start among its entries; returns the number of entries
__device__ inline uint32_t group_setup(const BudgetArgs& A, BudgetShared& sh) {
    const uint32_t t = threadIdx.x, g0 = blockIdx.x * kCompactGroup;
    __syncthreads();
    if (t < kCompactGroup) sh.tiles[t] = g0 + t < A.n_tiles ? A.tile[g0 + t] : make_uint2(0u, 0u);
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t q = 0; q < kCompactGroup; ++q) { sh.off[q] = run; run += sh.tiles[q].x; }
        sh.off[kCompactGroup] = run;
    }
    __syncthreads();
    return sh.off[kCompactGroup];
}

// entry e of the group, flattened: it belongs to the tile q with off[q] <= e < off[q + 1]
__device__ inline uint32_t group_entry(const BudgetArgs& A, const BudgetShared& sh, uint32_t e) {
    uint32_t q = 0;
#pragma unroll
    for (uint32_t k = 1; k < kCompactGroup; ++k) q += sh.off[k] <= e ? 1u : 0u;  // (empty tiles repeat an offset: counted past)
    return A.local[(size_t)sh.tiles[q].y + (e - sh.off[q])];
}

// a listed photon's key (one that is not < 0x7fffffff -- another key buffer than the selection was made from -- counts as the largest)
__device__ inline uint32_t listed_key(const BudgetArgs& A, uint32_t photon) {
    const uint32_t k = A.keys[photon];
    return k < kUnchanged ? k : kUnchanged;
}

// Histogram of digit LEVEL (0: bits 30..20, 1: bits 19..10, 2: bits 9..0) over the listed keys that agree with the cut in the
// digits above it: LDS histogram per workgroup, its non-zero bins added to the global table with integer atomics.  Does nothing
// when everything listed fits the budget (the short way) or the budget is 0.
template <int LEVEL>
__global__ __launch_bounds__(256) void budget_hist_kernel(BudgetArgs A) {
    constexpr uint32_t kBins = LEVEL == 0 ? kBins1 : (LEVEL == 1 ? kBins2 : kBins3);
    constexpr uint32_t kShift = LEVEL == 0 ? 20u : (LEVEL == 1 ? 10u : 0u);
    __shared__ BudgetShared sh;
    __shared__ uint32_t s_h[kBins];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t total = listed_total(A, sh);
    if (A.budget == 0u || total <= A.budget) return;
    uint32_t prefix = 0, rem = 0;
    derive_cut(A, LEVEL, sh, &prefix, &rem);
    for (uint32_t i = t; i < kBins; i += 256u) s_h[i] = 0u;
    (void)group_setup(A, sh);  // (its barriers also order the clearing of s_h before the adds)
    // tile by tile (a histogram does not care for the order: no search for an entry's tile as in the write launch)
    for (uint32_t q = 0; q < kCompactGroup; ++q)
    for (uint32_t base = 0; base < sh.tiles[q].x; base += 256u) {
        const uint32_t e = base + t;
        bool take = false;
        uint32_t d = 0;
        if (e < sh.tiles[q].x) {
            const uint32_t key = listed_key(A, A.local[(size_t)sh.tiles[q].y + e]);
            take = LEVEL == 0 || (key >> (kShift + 10u)) == prefix;
            d = (key >> kShift) & (kBins - 1u);
        }
        // equal keys are the common case (the equal-importance detector makes every key alike): one add per wave for the digit of its first taker
        const unsigned long long takers = __ballot(take);
        if (takers) {
            const uint32_t d0 = __shfl(d, __ffsll((long long)takers) - 1, 64);
            const unsigned long long same = __ballot(take && d == d0);
            if (take && d == d0) { if (lane == (uint32_t)(__ffsll((long long)same) - 1)) atomicAdd(&s_h[d0], (uint32_t)__popcll(same)); }
            else if (take) atomicAdd(&s_h[d], 1u);
        }
    }
    __syncthreads();
    uint32_t* table = A.hist + (LEVEL == 0 ? 0u : (LEVEL == 1 ? kBins1 : kBins1 + kBins2));
    for (uint32_t i = t; i < kBins; i += 256u) { const uint32_t c = s_h[i]; if (c) atomicAdd(&table[i], c); }
}

// per workgroup: its listed photons below the cut and on it
__global__ __launch_bounds__(256) void budget_count_kernel(BudgetArgs A) {
    __shared__ BudgetShared sh;
    const uint32_t t = threadIdx.x;
    const uint32_t total = listed_total(A, sh);
    if (A.budget == 0u || total <= A.budget) return;
    uint32_t T = 0, r = 0;
    derive_cut(A, 3, sh, &T, &r);
    (void)group_setup(A, sh);
    uint32_t lt = 0, eq = 0;
    for (uint32_t q = 0; q < kCompactGroup; ++q)
        for (uint32_t e = t; e < sh.tiles[q].x; e += 256u) {
            const uint32_t key = listed_key(A, A.local[(size_t)sh.tiles[q].y + e]);
            lt += key < T ? 1u : 0u;
            eq += key == T ? 1u : 0u;
        }
    lt = block_sum(lt, sh);
    eq = block_sum(eq, sh);
    if (t == 0) A.group[blockIdx.x] = make_uint2(lt, eq);
}

// The list.  Everything listed fits the budget: the tiles' lists lined up (selection_compact_kernel's result, bit for bit).
// Otherwise photon i is admitted when K[i] < T, or K[i] == T and fewer than r listed photons with that key precede it; its place
// is (admitted photons before it) = (listed photons below the cut before it) + min(r, ties before it) -- ascending, since the
// groups, their tiles and the tiles' lists are.  Workgroup 0 publishes m -> the device count word, and (epoch | m), (epoch | |C|)
// -> the host mailbox.
__global__ __launch_bounds__(256) void budget_write_kernel(BudgetArgs A, uint32_t* __restrict__ indices, int32_t* __restrict__ count_dev,
                                                           unsigned long long* mailbox, uint32_t epoch) {
    __shared__ BudgetShared sh;
    __shared__ uint32_t wcnt[2][4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t g0 = blockIdx.x * kCompactGroup;
    const uint32_t total = listed_total(A, sh);
    const bool all = total <= A.budget;
    if (blockIdx.x == 0 && t == 0) {
        const uint32_t m = all ? total : A.budget;
        *count_dev = (int32_t)m;
        __hip_atomic_store(mailbox + 1, ((unsigned long long)epoch << 32) | (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(mailbox, ((unsigned long long)epoch << 32) | (unsigned long long)m, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (A.budget == 0u) return;
    if (all) {
        uint32_t before = 0;
        for (uint32_t i = t; i < g0 && i < A.n_tiles; i += 256u) before += A.tile[i].x;
        before = block_sum(before, sh);
        const uint32_t entries = group_setup(A, sh);
        for (uint32_t e = t; e < entries; e += 256u) indices[before + e] = group_entry(A, sh, e);
        return;
    }
    uint32_t T = 0, r = 0;
    derive_cut(A, 3, sh, &T, &r);
    uint32_t lt_run = 0, eq_run = 0;  // listed photons below the cut / on it, ahead of this group (then: of the chunk)
    for (uint32_t g = t; g < blockIdx.x; g += 256u) { const uint2 c = A.group[g]; lt_run += c.x; eq_run += c.y; }
    lt_run = block_sum(lt_run, sh);
    eq_run = block_sum(eq_run, sh);
    const uint32_t entries = group_setup(A, sh);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base < entries; base += 256u) {
        const uint32_t e = base + t;
        uint32_t photon = 0;
        bool is_lt = false, is_eq = false;
        if (e < entries) {
            photon = group_entry(A, sh, e);
            const uint32_t key = listed_key(A, photon);
            is_lt = key < T;
            is_eq = key == T;
        }
        const unsigned long long bl = __ballot(is_lt), be = __ballot(is_eq);
        if (lane == 0) { wcnt[0][wave] = (uint32_t)__popcll(bl); wcnt[1][wave] = (uint32_t)__popcll(be); }
        __syncthreads();
        uint32_t lt_me = lt_run + (uint32_t)__popcll(bl & below), eq_me = eq_run + (uint32_t)__popcll(be & below);
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t cl = wcnt[0][w], ce = wcnt[1][w];
            lt_me += w < wave ? cl : 0u;
            eq_me += w < wave ? ce : 0u;
            lt_run += cl;
            eq_run += ce;
        }
        if (is_lt || (is_eq && eq_me < r)) {
            const uint32_t at = lt_me + (eq_me < r ? eq_me : r);
            if (at < A.budget) indices[at] = photon;  // (always, for keys that did not change under the passes)
        }
        __syncthreads();  // wcnt is rewritten by the next chunk
    }
}

}  // namespace

extern "C" {

int32_t cpm_update_budget(size_t n_photons, float percent) {
    if (!(percent > 0.f)) return 0;
    const float b = (percent / 100.f) * (float)n_photons;
    return b >= 2147483648.f ? INT32_MAX : (int32_t)b;
}

int cpm_selection_finish_budget(cpm_ctx* ctx, cpm_selection* s, const uint32_t* importances, int32_t budget, uint32_t* indices_out,
                                cpm_stream stream) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, s, "cpm_selection_finish_budget: null selection");
    CPM_REQUIRE(ctx, budget >= 0, "cpm_selection_finish_budget: negative budget");
    CPM_REQUIRE(ctx, !s->finished, "cpm_selection_finish_budget: already finished (cpm_selection_begin starts the next one)");
    CPM_REQUIRE(ctx, s->selections > 0, "cpm_selection_finish_budget: call cpm_selection_begin first");
    CPM_REQUIRE(ctx, s->n_launches == 0, "cpm_selection_finish_budget: a retrace launch has traced its photons already (use cpm_selection_finish)");
    CPM_REQUIRE(ctx, (importances && indices_out) || s->n_tiles == 0, "cpm_selection_finish_budget: null buffer");
    hipStream_t st = (hipStream_t)stream;
    s->last_stream = st;
    s->finished = true;
    ++s->epoch;
    // a selection one of whose calls failed selects nothing (as cpm_selection_finish)
    const uint32_t n_tiles = s->failed ? 0u : s->n_tiles;
    const BudgetArgs A{ s->tile, n_tiles, s->local, importances, (uint32_t)budget, s->budget_hist, s->budget_group };
    const dim3 grid(n_tiles ? (unsigned)div_up(n_tiles, kCompactGroup) : 1u), block(256);
    // the cut is only looked for when more photons than the budget CAN be listed (the device decides whether they are)
    if (n_tiles && budget > 0 && (size_t)budget < s->appended_photons) {
        CPM_HIP_CHECK(ctx, hipMemsetAsync(s->budget_hist, 0, kBudgetHistWords * sizeof(uint32_t), st));
        CPM_LAUNCH(ctx, budget_hist_kernel<0>, grid, block, 0, st, A);
        CPM_LAUNCH(ctx, budget_hist_kernel<1>, grid, block, 0, st, A);
        CPM_LAUNCH(ctx, budget_hist_kernel<2>, grid, block, 0, st, A);
        CPM_LAUNCH(ctx, budget_count_kernel, grid, block, 0, st, A);
    }
    CPM_LAUNCH(ctx, budget_write_kernel, grid, block, 0, st, A, indices_out, s->count_dev, s->mailbox_dev, s->epoch);
    CPM_LAUNCH_CHECK(ctx, "budget_write_kernel");
    if (s->failed)
        return set_error(ctx, CPM_ERR_DEVICE, "cpm_selection_finish_budget", "a select call of this selection failed: nothing is selected");
    return CPM_OK;
}

int cpm_selection_counts(cpm_ctx* ctx, cpm_selection* s, int32_t* n_selected, int32_t* n_changed) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, s && n_selected && n_changed, "cpm_selection_counts: null argument");
    *n_selected = *n_changed = 0;
    if (s->epoch == 0) return CPM_OK;  // nothing was ever selected
    // the finish's last launch writes word 1 (epoch | changed), then word 0 (epoch | listed) with release order
    const volatile unsigned long long* mb = s->mailbox;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
        const unsigned long long v0 = __atomic_load_n(mb, __ATOMIC_ACQUIRE);
        const unsigned long long v1 = __atomic_load_n(mb + 1, __ATOMIC_ACQUIRE);
        if ((uint32_t)(v0 >> 32) == s->epoch && (uint32_t)(v1 >> 32) == s->epoch) {
            *n_selected = (int32_t)(uint32_t)v0;
            *n_changed = (int32_t)(uint32_t)v1;
            return CPM_OK;
        }
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
        __builtin_ia32_pause();
    }
    // the mailbox did not arrive (a stream that is not running?): wait for the stream itself
    CPM_HIP_CHECK(ctx, hipStreamSynchronize(s->last_stream));
    const unsigned long long v0 = __atomic_load_n(mb, __ATOMIC_ACQUIRE), v1 = __atomic_load_n(mb + 1, __ATOMIC_ACQUIRE);
    CPM_REQUIRE(ctx, (uint32_t)(v0 >> 32) == s->epoch && (uint32_t)(v1 >> 32) == s->epoch, "cpm_selection_counts: the finish's mailbox words never arrived");
    *n_selected = (int32_t)(uint32_t)v0;
    *n_changed = (int32_t)(uint32_t)v1;
    return CPM_OK;
}

}  // extern "C"
