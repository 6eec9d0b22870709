// device_check.cpp -- the device resource layer (nafcodec_amd/csrc/device.cpp) on the CPU harness, alone: no decoder, no Python.
// Built by tests/test_device_emu.py from device.cpp + hipemu.cpp with -DNAFGPU_EMU -DNAFGPU_EMU_CACHE and
// -fsanitize=address,undefined: a freed buffer or a destroyed stream is poisoned memory, a kept one is not, and whatever
// is neither kept nor freed shows up as a leak at exit.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "device.h"

using namespace nafgpu;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "device_check:%d: %s\n", __LINE__, #cond);  \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static bool freed(const void *p) { return __asan_address_is_poisoned(p) != 0; }

int main() {
    CHECK(hipSetDevice(0) == hipSuccess);
    {   // 1. alloc: a smaller request keeps the buffer, a larger one replaces it; every byte asked for is there
        DevBuf b;
        CHECK(b.alloc(1000) && b.size() >= 1000);
        uint8_t *p = b.bytes();
        std::memset(p, 1, 1000);
        CHECK(b.alloc(500) && b.bytes() == p);
        CHECK(b.alloc(100000) && b.size() >= 100000 && b.bytes() != p && freed(p));
        std::memset(b.bytes(), 2, 100000);
        CHECK(b.alloc(size_t(1) << 20) && b.size() >= (size_t(1) << 20));      // above the size classes
        std::memset(b.bytes(), 3, size_t(1) << 20);
        CHECK(b.alloc(0) && b.bytes());
    }
    {   // 2. sizes that do not fit 63 bits are refused, not wrapped
        DevBuf b;
        CHECK(!b.alloc_items(1ull << 62, 8));
        CHECK(!b.alloc_items(1ull << 61, 2, 16));
        CHECK(b.alloc_items(10, 8, 16) && b.size() >= 96);
    }
    {   // 3. a view does not own what it points at
        DevBuf target, gone;
        CHECK(target.alloc(4096));
        {
            DevBuf v;
            v.view(target.bytes() + 16, 64);
            CHECK(v.bytes() == target.bytes() + 16 && v.size() == 64);
            v.release();
            CHECK(!v.bytes() && v.size() == 0 && !freed(target.bytes()));
            v.view(target.bytes(), 4096);                                      // ... nor when it dies as a view
        }
        CHECK(!freed(target.bytes()));
        CHECK(gone.alloc(4096));                                               // a view over an owner: the owned buffer is given up first
        uint8_t *q = gone.bytes();
        gone.view(target.bytes(), 8);
        CHECK(freed(q));
        std::memset(target.bytes(), 4, 4096);
    }
    uint8_t *kept = nullptr;
    {   // 4. a small buffer whose owner dies waits for the next one of its class; one given up by a living owner is freed
        DevBuf b;
        CHECK(b.alloc(300));
        uint8_t *p = b.bytes();
        b.release(true);
        CHECK(!b.bytes() && !freed(p));
        CHECK(b.alloc(300) && b.bytes() == p);
        b.release(false);
        CHECK(freed(p));
        CHECK(b.alloc(300) && b.bytes() != p);
        kept = b.bytes();
    }                                                                          // (~DevBuf: kept for the next taker)
    {   // 5. trim: the cache is emptied, and works again afterwards
        CHECK(!freed(kept));
        trim_device_memory(0);
        CHECK(freed(kept));
        trim_device_memory(0);
        trim_device_memory(-1);
        trim_device_memory(16);
        DevBuf b;
        CHECK(b.alloc(300));
        std::memset(b.bytes(), 5, 300);
    }
    {   // 6. streams: the one put is the one got; twelve idle ones are kept, the thirteenth is destroyed
        hipStream_t s = pooled_stream_get(0);
        CHECK(s);
        pooled_stream_put(0, s);
        CHECK(pooled_stream_get(0) == s);
        hipStream_t all[13] = {s};
        for (int i = 1; i < 13; i++) {
            all[i] = pooled_stream_get(0);
            CHECK(all[i]);
            for (int k = 0; k < i; k++) CHECK(all[k] != all[i]);
        }
        for (hipStream_t x : all) pooled_stream_put(0, x);
        for (int i = 0; i < 12; i++) CHECK(!freed(all[i]));
        CHECK(freed(all[12]));
        for (int i = 0; i < 12; i++) {                                         // (the last in is the first out)
            CHECK(pooled_stream_get(0) == all[11 - i]);
        }
        for (int i = 0; i < 12; i++) pooled_stream_put(0, all[i]);
        pooled_stream_put(0, nullptr);
        hipStream_t far = pooled_stream_get(16);                               // a device the pools do not know: plain calls
        CHECK(far);
        pooled_stream_put(16, far);
        CHECK(freed(far));
    }
    trim_device_memory(0);                                                     // what the last cases left in the cache
    std::puts("device_check: ok");
    return 0;
}
