// device.h -- device resources every front end shares (decoder, encoder, text parser, the C-ABI): buffers in HBM and what
// outlives their owners.  Per device, in one DeviceState (device.cpp): idle mapped ranges, idle small buffers, idle streams,
// the staging slots of large uploads.  Per process: the two pools of pinned HOST memory (PinnedBlocks, PinnedPool).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

namespace nafgpu {

inline bool hip_ok(hipError_t e) { return e == hipSuccess; }

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

class DevBuf {
public:
    DevBuf() = default;
    ~DevBuf() { release(true); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    bool alloc(size_t bytes);                 // contents undefined
    bool alloc_items(uint64_t count, uint64_t item_bytes, uint64_t extra_bytes = 0);   // count * item_bytes + extra_bytes, overflow-checked
    bool upload(const void *host, size_t bytes, hipStream_t stream);   // alloc + async H2D
    void release(bool dying = false);       // dying: the owner goes away (its streams are drained): a small buffer goes to the cache below
    void view(void *p, size_t bytes);         // a piece of another buffer: not owned, release() only forgets it
    template <class T>
    T *as() const { return static_cast<T *>(ptr_); }
    uint8_t *bytes() const { return static_cast<uint8_t *>(ptr_); }
    size_t size() const { return size_; }

private:
    bool alloc_mapped(size_t bytes);          // an address range backed by hipMemCreate chunks (device.cpp: why)
    void *ptr_ = nullptr;
    size_t size_ = 0, reserved_ = 0;          // reserved_ != 0: ptr_ is such a range
    bool view_ = false;
    bool small_ = false;                      // ptr_ is a size-class buffer (device.cpp: the small cache)
    int dev_ = -1;                            // the device that was current at alloc(): whose pools ptr_ came from and goes back to
#ifndef NAFGPU_EMU
    std::vector<hipMemGenericAllocationHandle_t> chunks_;
    size_t chunk_bytes_ = 0;                  // every chunk but the last maps this many bytes
#endif
};

// a stream of the pool that closed decoders leave theirs in (device.cpp: idle streams); the current device is `device`.
// put: the stream is synchronised and kept for the next taker
hipStream_t pooled_stream_get(int device);
void pooled_stream_put(int device, hipStream_t s);
// large host -> device copies, through the staging slots of the current device (device.cpp); returns when the bytes are across
bool upload_staged(uint8_t *d_dst, const uint8_t *src, size_t n, hipStream_t stream, size_t stage_min = 0);
void trim_device_memory(int device);             // the idle mapped ranges and small buffers of `device` go back to the driver

// Pinned host blocks for small read-backs (a copy into ordinary memory keeps its caller until it is done, 37 us apiece; into
// pinned memory it is enqueued in 5): blocks of 16 KiB, handed back when done, never freed.
constexpr size_t kPinnedBlock = size_t(16) << 10;
class PinnedBlocks {
public:
    static PinnedBlocks &instance() {
        static PinnedBlocks *p = new PinnedBlocks;
        return *p;
    }
    uint8_t *take() {
        {
            std::lock_guard<std::mutex> lock(mu_);
            if (!idle_.empty()) {
                uint8_t *p = idle_.back();
                idle_.pop_back();
                return p;
            }
        }
        void *p = nullptr;
        return hipHostMalloc(&p, kPinnedBlock) == hipSuccess ? static_cast<uint8_t *>(p) : nullptr;
    }
    void give(uint8_t *p) {
        if (!p) return;
        std::lock_guard<std::mutex> lock(mu_);
        idle_.push_back(p);
    }

private:
    std::mutex mu_;
    std::vector<uint8_t *> idle_;
};

// Pinned memory outlives decoders: hipHostMalloc + hipHostFree of the window were 1.5 of the 5 ms a 5-Mbase archive takes open to
// close (a caller that walks a directory of genomes pays them per file).  A closed decoder's windows go to a small per-process
// pool -- at most kPinnedPoolKeep buffers -- and the next decoder takes the smallest one that is large enough.
class PinnedPool {
public:
    static PinnedPool &instance() {
        static PinnedPool p;
        return p;
    }
    uint8_t *take(uint64_t want, uint64_t *cap) {
        std::lock_guard<std::mutex> g(mu_);
        int best = -1;
        for (int i = 0; i < n_; i++)
            if (cap_[i] >= want && (best < 0 || cap_[i] < cap_[best])) best = i;
        if (best < 0) return nullptr;
        uint8_t *p = buf_[best];
        *cap = cap_[best];
        buf_[best] = buf_[n_ - 1];
        cap_[best] = cap_[n_ - 1];
        n_--;
        return p;
    }
    void give(uint8_t *p, uint64_t cap) {
        {
            std::lock_guard<std::mutex> g(mu_);
            if (n_ < kPinnedPoolKeep) {
                buf_[n_] = p;
                cap_[n_] = cap;
                n_++;
                return;
            }
            int small = 0;                                 // full: the smallest buffer makes room for a larger one
            for (int i = 1; i < n_; i++)
                if (cap_[i] < cap_[small]) small = i;
            if (cap_[small] < cap) {
                std::swap(buf_[small], p);
                std::swap(cap_[small], cap);
            }
        }
        (void)hipHostFree(p);
    }

private:
    static constexpr int kPinnedPoolKeep = 4;
    std::mutex mu_;
    uint8_t *buf_[kPinnedPoolKeep] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t cap_[kPinnedPoolKeep] = {0, 0, 0, 0};
    int n_ = 0;
};

}  // namespace nafgpu
