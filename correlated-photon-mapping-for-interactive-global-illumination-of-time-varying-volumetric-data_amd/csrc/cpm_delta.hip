// cpm_delta.hip -- what a streamed time step sends when only part of the volume changes: the host pre-pass that encodes every transition
// of a host sequence as runs of changed 16-byte pieces (include/cpm/cpm_ext.h, "delta uploads"), and the kernel that patches such a
// delta into a device copy of the step before.
//
// The reference walks its host sequence on the CPU once before a step is shown (ref uniformgridcl/processors/
// dynamicvolumedifferenceanalysis.h:96-151, .cpp:60-104) and uploads whole elements (ref volumesequenceplayer.cpp:94-124).  At BASELINE
// config 5 (256^3 u8, the blob walking through the 32-step sequence) a transition changes 17 % of the pieces: 3 MiB of run table and
// payload instead of 16 MiB of PCIe.
#include <algorithm>
#include <chrono>
#include <new>
#include <thread>

#include "cpm_ctx.h"

using namespace cpm;

namespace {

constexpr uint64_t kPiece = 16;
constexpr int kMaxThreads = 16;   // the pre-pass's pool: a fixed cap, never the machine's core count

uint64_t round16(uint64_t n) { return (n + 15) & ~uint64_t(15); }

size_t step_bytes_of(const cpm_volume_desc* d) {
    return (size_t)d->dims[0] * d->dims[1] * d->dims[2] * cpm_dtype_size(d->dtype);
}

bool desc_ok(const cpm_volume_desc* d) {
    return d && cpm_dtype_valid(d->dtype) && d->dims[0] >= 1 && d->dims[1] >= 1 && d->dims[2] >= 1 &&
           (uint64_t)d->dims[0] * d->dims[1] * d->dims[2] * 4 <= kPiece * 0xffffffffull;
}

bool piece_differs(const uint8_t* a, const uint8_t* b, uint64_t p, uint64_t bytes) {
    const uint64_t at = p * kPiece;
    return memcmp(a + at, b + at, std::min(kPiece, bytes - at)) != 0;
}

// One walk over the pieces.  runs / payload may be null (sizing); stops early and returns false once the block would exceed `limit`.
bool encode(const uint8_t* from, const uint8_t* to, uint64_t bytes, uint64_t limit, uint32_t* runs, uint8_t* payload, uint32_t* n_runs_out,
            uint64_t* payload_bytes_out, uint64_t* dirty_out) {
    const uint64_t n_pieces = (bytes + kPiece - 1) / kPiece;
    uint32_t n_runs = 0;
    uint64_t dirty = 0, pay = 0;
    for (uint64_t p = 0; p < n_pieces;) {
        if (!piece_differs(from, to, p, bytes)) { ++p; continue; }
        const uint64_t first = p;
        while (p < n_pieces && piece_differs(from, to, p, bytes)) ++p;
        const uint64_t len = std::min(p * kPiece, bytes) - first * kPiece;
        if (runs) { runs[3 * n_runs] = (uint32_t)first; runs[3 * n_runs + 1] = (uint32_t)(p - first); runs[3 * n_runs + 2] = (uint32_t)dirty; }
        if (payload) memcpy(payload + pay, to + first * kPiece, len);
        ++n_runs; dirty += p - first; pay += len;
        if (round16(12ull * n_runs) + pay > limit) return false;
    }
    *n_runs_out = n_runs; *payload_bytes_out = pay; *dirty_out = dirty;
    return true;
}

void release(cpm_sequence_delta* d) {
    if (!d || --d->refs > 0) return;
    for (auto& t : d->transitions) if (t.block) (void)hipHostFree(t.block);
    delete d;
}

}  // namespace

// one lane per 16-byte payload piece, a workgroup per 256 of them.  The run of the workgroup's first piece: a 256-ary search over
// payload_piece_offset (each round one load per lane; how many of the sampled offsets are <= the piece names the next segment: two
// rounds at 40 K runs, where a lane's own binary search was a chain of 16 dependent L2 round trips -- 14 us for the launch).  The
// workgroup's pieces lie in at most 256 runs from there on: their offsets go to LDS and every lane finds its run there.  Then one 16-byte
// load and store; the short last piece of a block whose size is not a multiple of 16 is copied byte by byte (the volume's zeroed tail
// pad stays zero).  Every destination byte is written by exactly one lane: no atomics, the same bytes every launch.
__global__ void __launch_bounds__(256) delta_patch_kernel(const uint32_t* __restrict__ runs, uint32_t n_runs, const uint4* __restrict__ payload,
                                                          uint32_t n_payload_pieces, uint8_t* __restrict__ voxels, uint64_t bytes) {
    __shared__ uint32_t s_off[256], s_first[256];
    const uint32_t tid = threadIdx.x;
    for (uint32_t p0 = blockIdx.x * 256u; p0 < n_payload_pieces; p0 += gridDim.x * 256u) {
        uint32_t lo = 0, hi = n_runs;   // the run of p0 is in [lo, hi); offset[lo] <= p0
        while (hi - lo > 1) {
            const uint32_t stride = (hi - lo + 255) / 256, i = lo + tid * stride;
            const uint32_t c = (uint32_t)__syncthreads_count(i < hi && runs[3 * i + 2] <= p0);   // >= 1: sample 0 is lo
            lo += (c - 1) * stride;
            hi = min(lo + stride, hi);
        }
        const uint32_t n_here = min(n_runs - lo, 256u);
        if (tid < n_here) { s_off[tid] = runs[3 * (lo + tid) + 2]; s_first[tid] = runs[3 * (lo + tid)]; }
        __syncthreads();
        const uint32_t p = p0 + tid;
        if (p < n_payload_pieces) {
            uint32_t a = 0, b = n_here - 1;
            while (a < b) {
                const uint32_t mid = (a + b + 1) >> 1;
                if (s_off[mid] <= p) a = mid; else b = mid - 1;
            }
            const uint64_t at = ((uint64_t)s_first[a] + (p - s_off[a])) * 16;
            if (at + 16 <= bytes) {
                *reinterpret_cast<uint4*>(voxels + at) = payload[p];
            } else {
                const uint8_t* src = reinterpret_cast<const uint8_t*>(payload + p);
                for (uint64_t i = 0; at + i < bytes; ++i) voxels[at + i] = src[i];
            }
        }
        __syncthreads();   // (the next round refills s_off / s_first)
    }
}

namespace cpm {

int launch_delta_patch(cpm_ctx* ctx, const void* block_dev, uint32_t n_runs, uint64_t payload_bytes, void* voxels, uint64_t bytes, hipStream_t s) {
    if (n_runs == 0 || payload_bytes == 0) return CPM_OK;
    const uint64_t pieces = (payload_bytes + 15) / 16;
    CPM_REQUIRE(ctx, pieces < (1ull << 32) && payload_bytes <= bytes, "delta patch: block larger than the step");
    const uint8_t* base = static_cast<const uint8_t*>(block_dev);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((pieces + 255) / 256, 256ull * 32);
    CPM_LAUNCH(ctx, delta_patch_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(base), n_runs,
               reinterpret_cast<const uint4*>(base + round16(12ull * n_runs)), (uint32_t)pieces, static_cast<uint8_t*>(voxels), bytes);
    CPM_LAUNCH_CHECK(ctx, "delta_patch_kernel");
    return CPM_OK;
}

// (cpm_stream.hip: a stream's reference)
void sequence_delta_retain(cpm_sequence_delta* d) { ++d->refs; }
void sequence_delta_release(cpm_sequence_delta* d) { release(d); }

}  // namespace cpm

extern "C" {

int cpm_sequence_delta_encode(const cpm_volume_desc* desc, const void* from, const void* to, uint32_t* runs_out, void* payload_out,
                              size_t payload_capacity, uint32_t* n_runs, size_t* payload_bytes) {
    if (!desc_ok(desc) || !from || !to || !n_runs || !payload_bytes) return CPM_ERR_INVALID_ARGUMENT;
    const uint64_t bytes = step_bytes_of(desc);
    uint32_t nr = 0;
    uint64_t pay = 0, dirty = 0;
    (void)encode((const uint8_t*)from, (const uint8_t*)to, bytes, ~0ull, nullptr, nullptr, &nr, &pay, &dirty);
    *n_runs = nr; *payload_bytes = (size_t)pay;
    if (!runs_out) return CPM_OK;
    if (pay > payload_capacity || (pay && !payload_out)) return CPM_ERR_INVALID_ARGUMENT;
    (void)encode((const uint8_t*)from, (const uint8_t*)to, bytes, ~0ull, runs_out, (uint8_t*)payload_out, &nr, &pay, &dirty);
    return CPM_OK;
}

int cpm_sequence_delta_create(cpm_ctx* ctx, const cpm_volume_desc* desc, const void* const* host_steps, int n_steps, int wrap,
                              cpm_sequence_delta** out) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, out && host_steps && n_steps >= 2, "cpm_sequence_delta_create: bad argument");
    CPM_REQUIRE(ctx, desc_ok(desc), "cpm_sequence_delta_create: desc");
    for (int t = 0; t < n_steps; ++t) CPM_REQUIRE(ctx, host_steps[t], "cpm_sequence_delta_create: null step");
    *out = nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    cpm_sequence_delta* d = new (std::nothrow) cpm_sequence_delta();
    if (!d) return set_error(ctx, CPM_ERR_OUT_OF_MEMORY, "cpm_sequence_delta_create", "host allocation failed");
    d->desc = *desc; d->n_steps = n_steps; d->wrap = wrap ? 1 : 0;
    d->step_bytes = step_bytes_of(desc);
    const int n_tr = wrap ? n_steps : n_steps - 1;
    d->transitions.resize(n_steps);
    const uint64_t bytes = d->step_bytes, limit = bytes / 4 * 3 + (bytes % 4) * 3 / 4;
    const uint64_t n_pieces = (bytes + kPiece - 1) / kPiece;
    // workers: size every transition (stopping early past 3/4 of a step); the blocks are then pinned here and filled by the workers again
    std::vector<uint64_t> dirty(n_tr, 0);
    std::vector<char> full(n_tr, 0);
    const int n_threads = std::min(kMaxThreads, n_tr);
    auto run_pool = [&](auto&& body) {
        std::vector<std::thread> pool;
        for (int w = 0; w < n_threads; ++w)
            pool.emplace_back([&, w]() { for (int t = w; t < n_tr; t += n_threads) body(t); });
        for (auto& th : pool) th.join();
    };
    auto step = [&](int t) { return (const uint8_t*)host_steps[t]; };
    run_pool([&](int t) {
        auto& tr = d->transitions[t];
        uint64_t pay = 0;
        if (!encode(step(t), step((t + 1) % n_steps), bytes, limit, nullptr, nullptr, &tr.n_runs, &pay, &dirty[t])) {
            full[t] = 1;
            // the dirty count of a transition that is sent in full still goes into the mean
            uint64_t n = 0;
            for (uint64_t p = 0; p < n_pieces; ++p) n += piece_differs(step(t), step((t + 1) % n_steps), p, bytes);
            dirty[t] = n; tr.n_runs = 0;
            return;
        }
        tr.payload_bytes = pay;
        tr.bytes = round16(12ull * tr.n_runs) + pay;
    });
    int rc = CPM_OK;
    for (int t = 0; t < n_tr && rc == CPM_OK; ++t) {
        auto& tr = d->transitions[t];
        if (full[t]) continue;
        tr.stored = true;
        if (tr.bytes == 0) continue;
        hipError_t e = hipHostMalloc(&tr.block, tr.bytes, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); tr.block = nullptr; rc = set_error(ctx, CPM_ERR_OUT_OF_MEMORY, "hipHostMalloc(delta)", hipGetErrorString(e)); }
    }
    if (rc != CPM_OK) { release(d); return rc; }
    run_pool([&](int t) {
        auto& tr = d->transitions[t];
        if (!tr.block) return;
        uint8_t* blk = static_cast<uint8_t*>(tr.block);
        memset(blk + 12ull * tr.n_runs, 0, round16(12ull * tr.n_runs) - 12ull * tr.n_runs);
        uint32_t nr = 0;
        uint64_t pay = 0, dd = 0;
        (void)encode(step(t), step((t + 1) % n_steps), bytes, ~0ull, reinterpret_cast<uint32_t*>(blk), blk + round16(12ull * tr.n_runs), &nr, &pay, &dd);
    });
    double frac = 0.0;
    for (int t = 0; t < n_tr; ++t) frac += (double)dirty[t] / (double)std::max<uint64_t>(n_pieces, 1);
    d->dirty_fraction = frac / n_tr;
    d->analysis_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    *out = d;
    return CPM_OK;
}

int cpm_sequence_delta_get_info(cpm_ctx* ctx, const cpm_sequence_delta* d, cpm_sequence_delta_info* info) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, d && info, "cpm_sequence_delta_get_info: null argument");
    *info = cpm_sequence_delta_info{};
    info->n_steps = d->n_steps; info->wrap = d->wrap;
    info->n_transitions = d->wrap ? d->n_steps : d->n_steps - 1;
    info->step_bytes = d->step_bytes;
    for (int t = 0; t < info->n_transitions; ++t) {
        const auto& tr = d->transitions[t];
        if (!tr.stored) continue;
        ++info->n_delta_transitions;
        info->delta_bytes_total += tr.bytes;
        info->delta_bytes_max = std::max<uint64_t>(info->delta_bytes_max, tr.bytes);
    }
    info->dirty_fraction = d->dirty_fraction; info->analysis_ms = d->analysis_ms;
    return CPM_OK;
}

int cpm_sequence_delta_transition(cpm_ctx* ctx, const cpm_sequence_delta* d, int from, int to, uint32_t* n_runs, uint64_t* bytes) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, d && n_runs && bytes, "cpm_sequence_delta_transition: null argument");
    CPM_REQUIRE(ctx, from >= 0 && from < d->n_steps && to >= 0 && to < d->n_steps, "cpm_sequence_delta_transition: step out of range");
    CPM_REQUIRE(ctx, to == from + 1 || (d->wrap && from == d->n_steps - 1 && to == 0), "cpm_sequence_delta_transition: not a forward transition");
    const auto& tr = d->transitions[from];
    *n_runs = tr.stored ? tr.n_runs : 0;
    *bytes = tr.stored ? tr.bytes : d->step_bytes;
    return CPM_OK;
}

void cpm_sequence_delta_destroy(cpm_ctx* ctx, cpm_sequence_delta* d) {
    (void)ctx;
    release(d);
}

}  // extern "C"
