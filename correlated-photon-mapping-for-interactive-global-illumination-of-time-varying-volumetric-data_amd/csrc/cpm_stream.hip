// cpm_stream.hip -- a time-varying sequence whose steps live in HOST memory: the upload inside the step ("per step: upload
// volume, min/max, mean-abs-diff, ..."), hidden behind the step before it.
//
// The reference steps a host-side sequence: VolumeSequencePlayer::process picks two elements of a std::vector<std::shared_ptr<Volume>> and
// OpenGL uploads whichever is not resident yet (ref uniformgridcl/processors/volumesequenceplayer.cpp:94-124); the difference analysis walks
// the same elements on the CPU (ref uniformgridcl/processors/dynamicvolumedifferenceanalysis.h:96-151).  A sequence that does not stay on
// the device -- or has not been through its first loop -- pays 16 MiB of PCIe per 256^3 step: ~0.33 ms against a 0.07 ms correlated update.
//
// Here: a small ring of device volumes (linear block + the tracer's footprint copy each) over the host sequence, filled by a copy stream
// the library owns.  cpm_volume_stream_prefetch(tag, host voxels) enqueues, on that stream: wait until the consumer's work enqueued so far
// has drained (the slot it overwrites was last used there), H2D copy, footprint re-layout, an event; it returns at once.
// cpm_volume_stream_acquire(tag) makes the caller's stream wait for that event and hands the volume out.  A caller that prefetches step
// t + 1 before it acquires step t runs step t's min/max -> difference -> importance -> re-trace -> delta splat while step t + 1 crosses
// PCIe: the step costs max(upload, update), not their sum.  The host buffers should be pinned (cpm_pinned_alloc; hipMemcpyAsync from
// pageable memory is staged and blocks the host).
//
// With a cpm_sequence_delta attached (cpm_delta.hip) an upload whose step before is resident in another slot sends only what changed: the
// delta's block H2D into a staging buffer, then, once the victim is free, a device copy of that slot's linear block into the victim, the
// patch kernel and the same footprint re-layout -- about 3 MiB of PCIe instead of 16 at BASELINE config 5.  The H2D runs on a stream of
// its own into one of two staging buffers, so that step t + 1's block crosses PCIe while step t's copy, patch and re-layout run: the
// copy stream's step is then max(H2D, device work), not their sum (0.125 ms measured with one stream for both at config 5).
#include <new>

#include "cpm_ctx.h"

using namespace cpm;

struct cpm_volume_stream {
    static constexpr int kMaxSlots = 8;
    cpm_volume_desc desc;
    int device = 0, n_slots = 0;
    hipStream_t copy = nullptr;
    uint64_t clock = 0;
    struct Slot {
        cpm_volume* vol = nullptr;
        uint64_t tag = 0, last_use = 0;
        bool valid = false, timed = false, timed_delta = false;
        hipEvent_t ready = nullptr, fence = nullptr, t0 = nullptr, t1 = nullptr;
    } slots[kMaxSlots];
    // figures (cpm_volume_stream_stats)
    uint64_t uploads = 0, hits = 0, inline_uploads = 0, bytes = 0;
    double upload_ms = 0.0;   // H2D alone, from the events of the uploads that have finished
    uint64_t uploads_timed = 0;
    // delta uploads (cpm_volume_stream_use_delta): the delta, a device staging buffer for its largest block, the split of the figures
    cpm_sequence_delta* delta = nullptr;
    hipStream_t h2d = nullptr;                         // the blocks' H2D ...
    void* staging[2] = { nullptr, nullptr };           // ... into these in turn
    hipEvent_t staged[2] = { nullptr, nullptr };       // H2D into staging[k] done (h2d stream)
    hipEvent_t consumed[2] = { nullptr, nullptr };     // the patch that read staging[k] done (copy stream)
    int next_staging = 0;
    uint64_t delta_uploads = 0, full_uploads = 0, delta_bytes = 0, full_bytes = 0, delta_timed = 0;
    double delta_ms = 0.0;
};

namespace cpm {
void sequence_delta_retain(cpm_sequence_delta* d);
void sequence_delta_release(cpm_sequence_delta* d);
}

namespace {

void harvest(cpm_volume_stream* vs, cpm_volume_stream::Slot& sl) {
    if (!sl.timed || hipEventQuery(sl.t1) != hipSuccess) { (void)hipGetLastError(); return; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, sl.t0, sl.t1) == hipSuccess) {
        vs->upload_ms += ms; ++vs->uploads_timed;
        if (sl.timed_delta) { vs->delta_ms += ms; ++vs->delta_timed; }
    }
    (void)hipGetLastError();
    sl.timed = false;
}

cpm_volume_stream::Slot* find(cpm_volume_stream* vs, uint64_t tag) {
    for (int i = 0; i < vs->n_slots; ++i) if (vs->slots[i].valid && vs->slots[i].tag == tag) return &vs->slots[i];
    return nullptr;
}

// the stored transition into step `tag` whose step before sits in a slot other than the victim (its slot in *base), or nullptr: upload in full
const cpm_sequence_delta::Transition* delta_into(cpm_volume_stream* vs, uint64_t tag, const cpm_volume_stream::Slot* victim, cpm_volume_stream::Slot** base) {
    const cpm_sequence_delta* d = vs->delta;
    if (!d || tag >= (uint64_t)d->n_steps) return nullptr;
    if (tag == 0 && !d->wrap) return nullptr;
    const uint64_t from = tag == 0 ? (uint64_t)d->n_steps - 1 : tag - 1;
    const cpm_sequence_delta::Transition& tr = d->transitions[from];
    if (!tr.stored) return nullptr;
    *base = find(vs, from);
    if (!*base || *base == victim) return nullptr;
    return &tr;
}

int upload(cpm_ctx* ctx, cpm_volume_stream* vs, uint64_t tag, const void* host, hipStream_t consumer, cpm_volume_stream::Slot** out) {
    // the slot handed out longest ago (an empty one first)
    cpm_volume_stream::Slot* victim = nullptr;
    for (int i = 0; i < vs->n_slots; ++i) {
        cpm_volume_stream::Slot& s = vs->slots[i];
        if (!s.valid) { victim = &s; break; }
        if (!victim || s.last_use < victim->last_use) victim = &s;
    }
    harvest(vs, *victim);
    if (victim->timed) {   // (its last upload's events are still pending: they are recorded again below, so read them now)
        CPM_HIP_CHECK(ctx, hipEventSynchronize(victim->t1));
        harvest(vs, *victim);
    }
    cpm_volume* v = victim->vol;
    cpm_volume_stream::Slot* base = nullptr;
    const cpm_sequence_delta::Transition* tr = delta_into(vs, tag, victim, &base);
    int rc = CPM_OK;
    // (from here on the victim's contents are being replaced: it holds no step until the upload has been enqueued in full)
    victim->valid = false;
    if (tr) {
        // the block crosses PCIe first, on the h2d stream -- it waits neither for the consumer nor for the copy stream's work, only for the
        // patch that last read this staging buffer (two delta uploads ago)
        const int k = vs->next_staging;
        vs->next_staging ^= 1;
        CPM_HIP_CHECK(ctx, hipStreamWaitEvent(vs->h2d, vs->consumed[k], 0));
        CPM_HIP_CHECK(ctx, hipEventRecord(victim->t0, vs->h2d));
        if (tr->bytes) CPM_HIP_CHECK(ctx, hipMemcpyAsync(vs->staging[k], tr->block, tr->bytes, hipMemcpyHostToDevice, vs->h2d));
        CPM_HIP_CHECK(ctx, hipEventRecord(victim->t1, vs->h2d));
        CPM_HIP_CHECK(ctx, hipEventRecord(vs->staged[k], vs->h2d));
        CPM_HIP_CHECK(ctx, hipEventRecord(victim->fence, consumer));
        CPM_HIP_CHECK(ctx, hipStreamWaitEvent(vs->copy, victim->fence, 0));
        // the step before, complete: its own upload is earlier on the copy stream
        CPM_HIP_CHECK(ctx, hipMemcpyAsync(v->voxels, base->vol->voxels, v->bytes, hipMemcpyDeviceToDevice, vs->copy));
        CPM_HIP_CHECK(ctx, hipStreamWaitEvent(vs->copy, vs->staged[k], 0));
        rc = launch_delta_patch(ctx, vs->staging[k], tr->n_runs, tr->payload_bytes, v->voxels, v->bytes, vs->copy);
        if (rc) return rc;
        CPM_HIP_CHECK(ctx, hipEventRecord(vs->consumed[k], vs->copy));
    } else {
        // everything the consumer has enqueued so far may read the slot's old contents
        CPM_HIP_CHECK(ctx, hipEventRecord(victim->fence, consumer));
        CPM_HIP_CHECK(ctx, hipStreamWaitEvent(vs->copy, victim->fence, 0));
        CPM_HIP_CHECK(ctx, hipEventRecord(victim->t0, vs->copy));
        CPM_HIP_CHECK(ctx, hipMemcpyAsync(v->voxels, host, v->bytes, hipMemcpyHostToDevice, vs->copy));
        CPM_HIP_CHECK(ctx, hipEventRecord(victim->t1, vs->copy));
    }
    rc = build_quads(ctx, v, v->voxels, false, vs->copy);
    if (rc) return rc;
    CPM_HIP_CHECK(ctx, hipEventRecord(victim->ready, vs->copy));
    victim->tag = tag; victim->valid = true; victim->timed = true; victim->timed_delta = tr != nullptr;
    victim->last_use = ++vs->clock;
    ++vs->uploads;
    const uint64_t sent = tr ? tr->bytes : v->bytes;
    vs->bytes += sent;
    if (tr) { ++vs->delta_uploads; vs->delta_bytes += sent; }
    else if (vs->delta) { ++vs->full_uploads; vs->full_bytes += sent; }
    *out = victim;
    return CPM_OK;
}

}  // namespace

extern "C" {

int cpm_pinned_alloc(cpm_ctx* ctx, size_t bytes, void** out) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, out && bytes > 0, "cpm_pinned_alloc: bad argument");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return set_error(ctx, CPM_ERR_OUT_OF_MEMORY, "hipHostMalloc", hipGetErrorString(e)); }
    return CPM_OK;
}

void cpm_pinned_free(cpm_ctx* ctx, void* p) {
    (void)ctx;
    if (p) (void)hipHostFree(p);
}

int cpm_volume_stream_create(cpm_ctx* ctx, const cpm_volume_desc* desc, int n_slots, cpm_volume_stream** out) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, desc && out, "cpm_volume_stream_create: null argument");
    CPM_REQUIRE(ctx, n_slots >= 2 && n_slots <= cpm_volume_stream::kMaxSlots, "cpm_volume_stream_create: 2 to 8 slots");
    *out = nullptr;
    cpm_volume_stream* vs = new (std::nothrow) cpm_volume_stream();
    if (!vs) return set_error(ctx, CPM_ERR_OUT_OF_MEMORY, "cpm_volume_stream_create", "host allocation failed");
    vs->desc = *desc; vs->device = ctx->device; vs->n_slots = n_slots;
    bool ok = hipStreamCreateWithFlags(&vs->copy, hipStreamNonBlocking) == hipSuccess;
    int rc = CPM_OK;
    for (int i = 0; ok && i < n_slots; ++i) {
        cpm_volume_stream::Slot& s = vs->slots[i];
        rc = cpm_volume_create(ctx, desc, nullptr, 0, (cpm_stream)vs->copy, &s.vol);
        if (rc) break;
        ok = hipEventCreateWithFlags(&s.ready, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&s.fence, hipEventDisableTiming) == hipSuccess &&
             hipEventCreate(&s.t0) == hipSuccess && hipEventCreate(&s.t1) == hipSuccess;
    }
    if (rc || !ok) {
        (void)hipGetLastError();
        cpm_volume_stream_destroy(ctx, vs);
        return rc ? rc : set_error(ctx, CPM_ERR_DEVICE, "cpm_volume_stream_create", "stream / event creation failed");
    }
    *out = vs;
    return CPM_OK;
}

void cpm_volume_stream_destroy(cpm_ctx* ctx, cpm_volume_stream* vs) {
    if (!vs) return;
    (void)hipSetDevice(vs->device);
    if (vs->copy) (void)hipStreamSynchronize(vs->copy);
    if (vs->h2d) (void)hipStreamSynchronize(vs->h2d);
    for (auto& s : vs->slots) {
        for (hipEvent_t e : { s.ready, s.fence, s.t0, s.t1 }) if (e) (void)hipEventDestroy(e);
        if (s.vol) cpm_volume_destroy(ctx, s.vol);
    }
    if (vs->copy) (void)hipStreamDestroy(vs->copy);
    if (vs->h2d) (void)hipStreamDestroy(vs->h2d);
    for (int k = 0; k < 2; ++k) {
        if (vs->staging[k]) (void)hipFree(vs->staging[k]);
        for (hipEvent_t e : { vs->staged[k], vs->consumed[k] }) if (e) (void)hipEventDestroy(e);
    }
    if (vs->delta) sequence_delta_release(vs->delta);
    delete vs;
}

int cpm_volume_stream_prefetch(cpm_ctx* ctx, cpm_volume_stream* vs, uint64_t tag, const void* host_voxels, cpm_stream consumer) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, vs && host_voxels, "cpm_volume_stream_prefetch: null argument");
    cpm_volume_stream::Slot* s = find(vs, tag);
    if (s) { s->last_use = ++vs->clock; return CPM_OK; }   // (about to be used: not the next upload's victim)
    return upload(ctx, vs, tag, host_voxels, (hipStream_t)consumer, &s);
}

int cpm_volume_stream_acquire(cpm_ctx* ctx, cpm_volume_stream* vs, uint64_t tag, const void* host_voxels, cpm_stream consumer, cpm_volume** out) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, vs && out, "cpm_volume_stream_acquire: null argument");
    *out = nullptr;
    cpm_volume_stream::Slot* s = find(vs, tag);
    if (s) ++vs->hits;
    else {
        CPM_REQUIRE(ctx, host_voxels, "cpm_volume_stream_acquire: the step is not resident and no host voxels were given");
        int rc = upload(ctx, vs, tag, host_voxels, (hipStream_t)consumer, &s);
        if (rc) return rc;
        ++vs->inline_uploads;
    }
    CPM_HIP_CHECK(ctx, hipStreamWaitEvent((hipStream_t)consumer, s->ready, 0));
    s->last_use = ++vs->clock;
    *out = s->vol;
    return CPM_OK;
}

int cpm_volume_stream_stats(cpm_ctx* ctx, cpm_volume_stream* vs, cpm_volume_stream_info* info) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, vs && info, "cpm_volume_stream_stats: null argument");
    for (int i = 0; i < vs->n_slots; ++i) harvest(vs, vs->slots[i]);
    info->uploads = vs->uploads; info->hits = vs->hits; info->uploads_at_acquire = vs->inline_uploads; info->bytes_uploaded = vs->bytes;
    info->uploads_timed = vs->uploads_timed; info->upload_ms_total = vs->upload_ms;
    info->bytes_per_step = vs->n_slots ? vs->slots[0].vol->bytes : 0;
    return CPM_OK;
}

int cpm_volume_stream_use_delta(cpm_ctx* ctx, cpm_volume_stream* vs, cpm_sequence_delta* delta) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, vs && delta, "cpm_volume_stream_use_delta: null argument");
    CPM_REQUIRE(ctx, !vs->delta && vs->uploads == 0, "cpm_volume_stream_use_delta: the stream has a delta or has uploaded steps already");
    CPM_REQUIRE(ctx, delta->desc.dtype == vs->desc.dtype && delta->desc.dims[0] == vs->desc.dims[0] && delta->desc.dims[1] == vs->desc.dims[1] &&
                     delta->desc.dims[2] == vs->desc.dims[2], "cpm_volume_stream_use_delta: the delta's steps are not the stream's");
    uint64_t most = 0;
    for (const auto& tr : delta->transitions) if (tr.stored) most = std::max<uint64_t>(most, tr.bytes);
    // (what is created here is released by cpm_volume_stream_destroy, also when a step below fails)
    for (int k = 0; k < 2; ++k) {
        if (vs->staging[k]) { (void)hipFree(vs->staging[k]); vs->staging[k] = nullptr; }
        hipError_t e = hipMalloc(&vs->staging[k], most + 64);   // (+ the 16-byte read of a short last piece)
        if (e != hipSuccess) { (void)hipGetLastError(); vs->staging[k] = nullptr; return set_error(ctx, CPM_ERR_OUT_OF_MEMORY, "hipMalloc(delta staging)", hipGetErrorString(e)); }
        if (!vs->staged[k]) CPM_HIP_CHECK(ctx, hipEventCreateWithFlags(&vs->staged[k], hipEventDisableTiming));
        if (!vs->consumed[k]) CPM_HIP_CHECK(ctx, hipEventCreateWithFlags(&vs->consumed[k], hipEventDisableTiming));
        CPM_HIP_CHECK(ctx, hipEventRecord(vs->consumed[k], vs->copy));   // (nothing has read it yet)
    }
    if (!vs->h2d) CPM_HIP_CHECK(ctx, hipStreamCreateWithFlags(&vs->h2d, hipStreamNonBlocking));
    sequence_delta_retain(delta);
    vs->delta = delta;
    return CPM_OK;
}

int cpm_volume_stream_delta_stats(cpm_ctx* ctx, cpm_volume_stream* vs, cpm_volume_stream_delta_info* info) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, vs && info, "cpm_volume_stream_delta_stats: null argument");
    for (int i = 0; i < vs->n_slots; ++i) harvest(vs, vs->slots[i]);
    info->delta_uploads = vs->delta_uploads; info->full_uploads = vs->full_uploads;
    info->delta_bytes = vs->delta_bytes; info->full_bytes = vs->full_bytes;
    info->delta_uploads_timed = vs->delta_timed; info->delta_h2d_ms_total = vs->delta_ms;
    return CPM_OK;
}

}  // extern "C"
