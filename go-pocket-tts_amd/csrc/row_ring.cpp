// row_ring.cpp -- RingAck (row_ring.h): the hand-back of a ring turn's sequence number and the host's wait for it.
#include <chrono>
#include <thread>

#include "row_ring.h"

namespace ptts {

RingAck::~RingAck() {
    if (back) (void)hipHostFree(back);
}

void RingAck::wait(int t) {
    if (!expect[t]) return;
    const volatile uint64_t* p = back + t;
    if (*p == expect[t]) return;
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0; *p != expect[t]; spins++) {
        if (spins < 256) continue;
        std::this_thread::yield();
        if ((spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))
            throw Error(PTTS_ENODEVICE, "ptts-hip: a row table's launches did not finish within 60 s");
    }
}

void RingAck::upload(int t, char* host_turn, char* dev_turn, size_t row_bytes, hipStream_t s) {
    if (!back) {
        PTTS_HIP(hipHostMalloc((void**)&back, sizeof(uint64_t) * kRing, hipHostMallocDefault));
        std::memset(back, 0, sizeof(uint64_t) * kRing);
    }
    expect[t] = ++seq;
    std::memcpy(host_turn, &expect[t], sizeof(uint64_t));
    PTTS_HIP(hipMemcpyAsync(dev_turn, host_turn, kHead + row_bytes, hipMemcpyHostToDevice, s));
}

void RingAck::done(int t, const char* dev_turn, hipStream_t s) {
    PTTS_HIP(hipMemcpyAsync(back + t, dev_turn, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
}

}  // namespace ptts
