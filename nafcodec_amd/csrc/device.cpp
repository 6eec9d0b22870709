// device.cpp -- see device.h
#include "device.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "kernels.h"

namespace nafgpu {

static std::atomic<bool> g_test_hooks{false};
void set_test_hooks(bool on) { g_test_hooks.store(on); }
const char *hook_env(const char *name) { return g_test_hooks.load() ? std::getenv(name) : nullptr; }

#if !defined(NAFGPU_EMU) || defined(NAFGPU_EMU_CACHE)   // (NAFGPU_EMU_CACHE: a harness build WITH the cache, to chase what depends on it)
#define NAFGPU_SMALL_CACHE 1
#endif

// ------------------------------------------------------------------ what a device keeps: one DeviceState each
namespace {
#ifndef NAFGPU_EMU
// Large buffers come from the virtual-memory API: an address range backed by hipMemCreate chunks of up to 1 GiB.  Why: memory
// from one large hipMalloc writes at 4.9-6.7 TB/s depending on the allocation (the same virtual address after a hipFree can
// land on either side; tools/frontbench4.hip, profiles/r03_frontbench4.log -- a plain streaming fill shows it as well as
// K1's 610 k write fronts), which is what made K1 take 10.7-11.9 ms on the same archive.  Chunked backing gave 6.7 TB/s in
// nine allocations out of nine, whatever the chunk size (2 MiB, 64 MiB, 1 GiB).
constexpr size_t kVmmMinBytes = size_t(32) << 20, kVmmChunk = size_t(1) << 30;

// Mapped ranges outlive the buffers they were.  Unmapping a range and mapping memory at the same addresses a moment later is
// (a) slow -- the address ranges and chunks of a 50 GB decoder take 10 ms in one process and 0.3-0.8 s in the next -- and
// (b) NOT SAFE on this stack: a decoder that went from tiles to the whole output (its 2 GiB tile buffer unmapped and freed,
// buffers of 4.4 GB and 1.1 GB reserved and mapped in the same call, the smaller one at the addresses just freed) found
// about every other 4 KiB page of its freshly uploaded source bytes holding something else -- zeros where the chunks were
// new, old bytes where they were reused (NAFGPU_DEBUG_VERIFY_UPLOAD; plain hipMalloc: fine; unmapping chunk by chunk and
// keeping the chunks for reuse: no better).  Translations of the old mapping seem to outlive it.  So a released range stays
// as it is -- reserved, mapped, its chunks in place -- and waits here for the next buffer of its size (sizes are multiples of
// kVmmTail, so that they meet their like again; a range up to an eighth larger than asked for is taken too).  When a creation
// fails for want of memory the idle ranges are unmapped and their chunks released, but their ADDRESSES are never given back:
// no later mapping can land where an old one was.
constexpr size_t kVmmTail = size_t(64) << 20;
struct IdleRange {
    void *va;
    size_t total, chunk;
    std::vector<hipMemGenericAllocationHandle_t> chunks;
};
// idle ranges kept per device at most (the oldest go first).  Not more: a process that holds -- or has just given back -- a hundred
// gigabytes makes the NEXT process's first allocations take 0.5 s longer (bench.py's iterator legs run in children)
constexpr size_t kVmmKeepBytes = size_t(16) << 30;

// The slots of a staged upload (upload_staged below): a stream, two pinned buffers and the events behind which they are reused
constexpr size_t kStageChunk = size_t(16) << 20;
constexpr unsigned kStageThreads = 8;
constexpr size_t kStageMin = size_t(256) << 20;            // smaller uploads: one plain copy
struct StageSlot {
    uint8_t *buf[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    hipEvent_t done[2] = {nullptr, nullptr};
};
#endif

#ifdef NAFGPU_SMALL_CACHE
// Small device buffers outlive their decoders.  Opening, decoding and closing one of the reference's fixtures makes a hundred
// hipMalloc calls and as many hipFree calls, each of which waits for the device (rocprofv3 --hip-trace, tools/small_api_trace.sh:
// 0.75 ms of a 3.6 ms cycle): buffers of up to 256 KiB come in power-of-two size classes, and one whose OWNER goes away (the
// destructor: by then the owner's streams are drained, ~ArchiveJob) is kept for the next decoder on the same device -- up to
// 64 MiB of them per device.  A buffer given up while its owner lives on (alloc() growing it) is freed as before: hipFree's wait
// is what makes that safe.  The CPU harness does without: rounded-up sizes would hide small overruns from the sanitizer.
constexpr size_t kSmallMax = size_t(256) << 10, kSmallMin = 256, kSmallKeepBytes = size_t(64) << 20;
constexpr int kSmallClasses = 11;                          // 256 B .. 256 KiB
int small_class(size_t bytes) {
    int c = 0;
    while ((kSmallMin << c) < bytes) c++;
    return c;
}
#endif

// Streams outlive decoders.  hipStreamCreate takes 2.7 ms and hipStreamDestroy 2.4 ms on this stack (rocprofv3 --hip-trace of
// tools/small_probe.py: 80 % of the 14-18 ms that opening, decoding and closing ONE of the reference's fixtures took, whatever
// its size -- a decoder owns three streams), so a closed decoder hands its streams to the next one on the same device.  A
// stream is idle when it comes back (synchronised), and a few per device are kept.
constexpr size_t kStreamKeep = 12;
constexpr int kMaxDevices = 16;                            // devices that pool; any other gets the plain calls

// Everything idle that belongs to one device.  Never torn down (new, not static objects): at process exit the runtime may be
// gone before a static destructor runs.
struct DeviceState {
    std::mutex mu;                                         // the three idle lists
    std::vector<hipStream_t> streams;
#ifdef NAFGPU_SMALL_CACHE
    std::vector<void *> small[kSmallClasses];
    size_t small_bytes = 0;
#endif
#ifndef NAFGPU_EMU
    std::vector<IdleRange> ranges;
    std::mutex stage_mu;                                   // one staged upload at a time per device (the buffers are shared)
    StageSlot stage[kStageThreads];
    bool stage_ready = false, stage_failed = false;
#endif
};
DeviceState *device_state(int dev) {                       // null: no pooling, the caller falls through to the plain call
    static DeviceState *const states = new DeviceState[kMaxDevices];
    return dev >= 0 && dev < kMaxDevices ? &states[dev] : nullptr;
}
int current_device() {
    int dev = -1;
    return hip_ok(hipGetDevice(&dev)) ? dev : -1;
}

#ifndef NAFGPU_EMU
// memory back to the driver, chunk by chunk as it was mapped; the addresses stay reserved
void unmap_chunks(void *va, size_t total, size_t chunk, const std::vector<hipMemGenericAllocationHandle_t> &chunks) {
    size_t k = 0;
    for (size_t off = 0; off < total; off += chunk, k++) {
        (void)hipMemUnmap(static_cast<char *>(va) + off, std::min(chunk, total - off));
        if (k < chunks.size()) (void)hipMemRelease(chunks[k]);
    }
}
bool range_take(DeviceState &ds, size_t total, size_t chunk, IdleRange *out) {
    std::lock_guard<std::mutex> lock(ds.mu);
    auto &v = ds.ranges;
    size_t best = v.size();
    for (size_t i = 0; i < v.size(); i++)
        if (v[i].chunk == chunk && v[i].total >= total && v[i].total - total <= total / 8 && (best == v.size() || v[i].total < v[best].total)) best = i;
    if (best == v.size()) return false;
    *out = std::move(v[best]);
    v.erase(v.begin() + static_cast<std::ptrdiff_t>(best));
    return true;
}
void range_give(DeviceState &ds, IdleRange &&r) {
    std::lock_guard<std::mutex> lock(ds.mu);
    auto &v = ds.ranges;
    v.push_back(std::move(r));
    size_t held = 0;
    for (const IdleRange &e : v) held += e.total;
    while (held > kVmmKeepBytes && v.size() > 1) {
        held -= v.front().total;
        unmap_chunks(v.front().va, v.front().total, v.front().chunk, v.front().chunks);
        v.erase(v.begin());
    }
}
void range_trim(DeviceState &ds) {                         // the memory of everything idle goes back to the driver (not the addresses)
    std::lock_guard<std::mutex> lock(ds.mu);
    for (IdleRange &r : ds.ranges) unmap_chunks(r.va, r.total, r.chunk, r.chunks);
    ds.ranges.clear();
}
bool stage_init(DeviceState &ds) {                         // (under ds.stage_mu)
    if (ds.stage_ready) return true;
    if (ds.stage_failed) return false;
    for (StageSlot &sl : ds.stage) {
        bool ok = hipStreamCreate(&sl.stream) == hipSuccess;
        for (int k = 0; k < 2 && ok; k++)
            ok = hipHostMalloc(reinterpret_cast<void **>(&sl.buf[k]), kStageChunk) == hipSuccess &&
                 hipEventCreateWithFlags(&sl.done[k], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            ds.stage_failed = true;                        // (what was allocated stays: a plain copy serves from here on)
            return false;
        }
    }
    ds.stage_ready = true;
    return true;
}
#endif

// allocate, and on failure let the device's idle ranges give their memory back and try once more
template <class F>
bool alloc_retry(DeviceState *ds, F attempt) {
    if (attempt()) return true;
#ifndef NAFGPU_EMU
    (void)hipGetLastError();
    if (ds) {
        range_trim(*ds);
        return attempt();
    }
#endif
    return false;
}
}  // namespace

// ------------------------------------------------------------------ DevBuf
bool DevBuf::alloc_items(uint64_t count, uint64_t item_bytes, uint64_t extra_bytes) {
    // sizes derived from untrusted header fields: refuse anything that does not fit 63 bits instead of wrapping
    if (item_bytes && count > ((1ull << 62) - extra_bytes) / item_bytes) return false;
    return alloc(static_cast<size_t>(count * item_bytes + extra_bytes));
}

#ifndef NAFGPU_EMU
bool DevBuf::alloc_mapped(size_t bytes) {
    DeviceState *ds = device_state(dev_);
    int vmm = 0;
    size_t gran = 0;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev_;
    if (!ds || !hip_ok(hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, dev_)) || !vmm ||
        !hip_ok(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended)) || !gran || kVmmChunk % gran)
        return false;
    size_t chunk = kVmmChunk;
    if (const char *ce = hook_env("NAFGPU_VMM_CHUNK_MIB")) {        // (experiments: tools/placement_probe.sh)
        const size_t want = static_cast<size_t>(std::strtoull(ce, nullptr, 10)) << 20;
        if (want >= gran && want % gran == 0) chunk = want;
    }
    const size_t tail_unit = kVmmTail % gran == 0 && chunk % kVmmTail == 0 ? kVmmTail : gran;
    const size_t total = (bytes + tail_unit - 1) / tail_unit * tail_unit;
    IdleRange r{nullptr, total, chunk, {}};
    if (hook_env("NAFGPU_VMM_NO_POOL") || !range_take(*ds, total, chunk, &r)) {   // nothing idle of this size: a new range
        if (!hip_ok(hipMemAddressReserve(&r.va, total, gran, nullptr, 0)) || !r.va) return false;
        size_t mapped = 0;
        bool ok = true;
        for (size_t off = 0; off < total && ok; off += chunk) {
            const size_t n = total - off < chunk ? total - off : chunk;
            hipMemGenericAllocationHandle_t h;
            // (what waits for a buffer of another size gives its memory back first)
            if (!alloc_retry(ds, [&] { return hip_ok(hipMemCreate(&h, n, &prop, 0)); })) { ok = false; break; }
            if (!hip_ok(hipMemMap(static_cast<char *>(r.va) + off, n, 0, h, 0))) {
                (void)hipMemRelease(h);
                ok = false;
                break;
            }
            r.chunks.push_back(h);
            mapped = off + n;
        }
        if (ok) {
            hipMemAccessDesc acc = {};
            acc.location = prop.location;
            acc.flags = hipMemAccessFlagsProtReadWrite;
            ok = hip_ok(hipMemSetAccess(r.va, total, &acc, 1));
        }
        if (!ok) {                               // e.g. out of device memory: undo, the caller reports the failure of hipMalloc
            unmap_chunks(r.va, mapped, chunk, r.chunks);
            (void)hipMemAddressFree(r.va, total);
            (void)hipGetLastError();
            return false;
        }
    }
    ptr_ = r.va;
    size_ = bytes;
    reserved_ = r.total;
    chunk_bytes_ = r.chunk;
    chunks_ = std::move(r.chunks);
    return true;
}
#endif

void DevBuf::view(void *p, size_t bytes) {
    release();
    ptr_ = p;
    size_ = bytes;
    view_ = true;
}

bool DevBuf::alloc(size_t bytes) {
    if (ptr_ && !view_ && bytes <= size_) return true;
    release();
    dev_ = current_device();
    // (nafgpu_test_hooks + NAFGPU_ALLOC_PLAIN=1: everything from hipMalloc, for A/B runs -- tools/placement_probe.sh; any value:
    //  no small-buffer cache)
    [[maybe_unused]] const char *plain = hook_env("NAFGPU_ALLOC_PLAIN");
#ifndef NAFGPU_EMU
    if (bytes >= kVmmMinBytes && !(plain && plain[0] == '1') && alloc_mapped(bytes)) return true;
#endif
    DeviceState *ds = device_state(dev_);
    size_t want = bytes ? bytes : 16;
    void *p = nullptr;
#ifdef NAFGPU_SMALL_CACHE
    if (bytes <= kSmallMax && !plain && ds) {              // a size class: a buffer that waits for its next owner, or a new one
        const int c = small_class(bytes);
        want = kSmallMin << c;
        small_ = true;
        std::lock_guard<std::mutex> lock(ds->mu);
        if (!ds->small[c].empty()) {
            p = ds->small[c].back();
            ds->small[c].pop_back();
            ds->small_bytes -= want;
        }
    }
#endif
    // (idle ranges give their memory back before anything fails for want of it)
    if (!p && !alloc_retry(ds, [&] { return hip_ok(hipMalloc(&p, want)); })) return false;
    ptr_ = p;
    size_ = want;
    return true;
}

bool DevBuf::upload(const void *host, size_t bytes, hipStream_t stream) {
    if (!alloc(bytes)) return false;
    if (bytes == 0) return true;
    return hip_ok(hipMemcpyAsync(ptr_, host, bytes, hipMemcpyHostToDevice, stream));
}

void DevBuf::release(bool dying) {
    if (view_) ptr_ = nullptr;                             // (not owned: only forgotten)
    view_ = false;
#ifdef NAFGPU_SMALL_CACHE
    if (DeviceState *ds = ptr_ && small_ && dying ? device_state(dev_) : nullptr) {   // kept for the next owner, if there is room
        std::lock_guard<std::mutex> lock(ds->mu);
        if (ds->small_bytes + size_ <= kSmallKeepBytes) {
            ds->small[small_class(size_)].push_back(ptr_);
            ds->small_bytes += size_;
            ptr_ = nullptr;
        }
    }
#endif
#ifndef NAFGPU_EMU
    if (ptr_ && reserved_) {
        // (IdleRange above: why the range is kept as it is rather than unmapped)
        const size_t step = chunk_bytes_ ? chunk_bytes_ : reserved_;
        DeviceState *ds = device_state(dev_);
        if (ds && !hook_env("NAFGPU_VMM_NO_POOL")) {
            if (!dying) (void)hipDeviceSynchronize();      // (a living owner: whatever it still has in flight is done before another takes the range)
            range_give(*ds, IdleRange{ptr_, reserved_, step, std::move(chunks_)});
        } else {
            if (hook_env("NAFGPU_VMM_SYNC_UNMAP")) (void)hipDeviceSynchronize();   // (experiment: is anything still in flight on the range?)
            unmap_chunks(ptr_, reserved_, step, chunks_);
            (void)hipMemAddressFree(ptr_, reserved_);
        }
        chunks_.clear();
        ptr_ = nullptr;
    }
#endif
    if (ptr_) (void)hipFree(ptr_);
    ptr_ = nullptr;
    size_ = reserved_ = 0;
    small_ = false;
}

void trim_device_memory(int device) {
    DeviceState *ds = device_state(device);
    if (!ds) return;
#ifndef NAFGPU_EMU
    (void)hipDeviceSynchronize();
    range_trim(*ds);
#endif
#ifdef NAFGPU_SMALL_CACHE
    std::vector<void *> gone[kSmallClasses];
    {
        std::lock_guard<std::mutex> lock(ds->mu);
        std::swap(gone, ds->small);
        ds->small_bytes = 0;
    }
    for (const std::vector<void *> &v : gone)
        for (void *p : v) (void)hipFree(p);
#endif
}

// ------------------------------------------------------------------ large uploads
// Host -> device for the compressed bytes of a section.  One hipMemcpyAsync out of ordinary or mapped memory moves at PCIe rate in
// one process and at a quarter of it in the next -- the runtime's copy engines again (see k_copy_out: 10 GB in 0.2 s or in 1.2 s,
// tools/iter_regime_probe.py) -- so large uploads take the same road as the read-back: kStageThreads host threads copy their
// chunks of the source into pinned buffers (two of 16 MiB each, so the memcpy of one overlaps the transfer of the other; the
// page faults of a file mapping spread over the threads as well), and the GPU fetches every chunk itself (k_copy_out with
// the pinned buffer as its source).  The slots -- and so the streams k_copy_out runs on -- are those of the current device,
// which owns the destination; they are created there on first use.  Returns when every byte is on the device.
bool upload_staged(uint8_t *d_dst, const uint8_t *src, size_t n, hipStream_t stream, size_t stage_min) {
#ifndef NAFGPU_EMU
    const int dev = current_device();
    DeviceState *ds = device_state(dev);
    if (ds && n >= (stage_min ? stage_min : kStageMin) && !hook_env("NAFGPU_NO_STAGING")) {
        std::lock_guard<std::mutex> guard(ds->stage_mu);
        if (stage_init(*ds) && hipStreamSynchronize(stream) == hipSuccess) {   // (what was enqueued in front -- the pad memsets -- is done)
            const size_t n_chunks = (n + kStageChunk - 1) / kStageChunk;
            std::atomic<bool> failed{false};
            const bool sdma = hook_env("NAFGPU_STAGE_SDMA") != nullptr;   // (experiment: the copy engines fetch the chunks, not a kernel)
            auto worker = [&](unsigned t) {
                (void)hipSetDevice(dev);
                StageSlot &sl = ds->stage[t];
                unsigned k = 0;
                for (size_t c = t; c < n_chunks && !failed.load(); c += kStageThreads, k ^= 1u) {
                    const size_t off = c * kStageChunk, len = std::min(kStageChunk, n - off);
                    if (hipEventSynchronize(sl.done[k]) != hipSuccess) failed = true;   // (the kernel that last read this buffer)
                    std::memcpy(sl.buf[k], src + off, len);
                    if (sdma) {
                        if (hipMemcpyAsync(d_dst + off, sl.buf[k], len, hipMemcpyHostToDevice, sl.stream) != hipSuccess) failed = true;
                    } else {
                        launch_copy_out(sl.stream, d_dst + off, sl.buf[k], len);
                    }
                    if (hipGetLastError() != hipSuccess || hipEventRecord(sl.done[k], sl.stream) != hipSuccess) failed = true;
                }
                if (hipStreamSynchronize(sl.stream) != hipSuccess) failed = true;
            };
            std::vector<std::thread> pool;
            unsigned started = 1;
            try {
                for (; started < kStageThreads; started++) pool.emplace_back(worker, started);
            } catch (...) {                                // no more threads to be had: their chunks are done here
            }
            worker(0);
            for (unsigned t = started; t < kStageThreads; t++) worker(t);
            for (std::thread &th : pool) th.join();
            return !failed.load();
        }
    }
#endif
    return hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, stream) == hipSuccess;
}

// ------------------------------------------------------------------ streams
hipStream_t pooled_stream_get(int device) {
    if (DeviceState *ds = device_state(device)) {
        std::lock_guard<std::mutex> lock(ds->mu);
        if (!ds->streams.empty()) {
            hipStream_t s = ds->streams.back();
            ds->streams.pop_back();
            return s;
        }
    }
    hipStream_t s = nullptr;
    return hip_ok(hipStreamCreate(&s)) ? s : nullptr;
}

void pooled_stream_put(int device, hipStream_t s) {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    if (DeviceState *ds = device_state(device)) {
        std::lock_guard<std::mutex> lock(ds->mu);
        if (ds->streams.size() < kStreamKeep) {
            ds->streams.push_back(s);
            return;
        }
    }
    (void)hipStreamDestroy(s);
}

}  // namespace nafgpu
