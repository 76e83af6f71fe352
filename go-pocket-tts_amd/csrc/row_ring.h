// row_ring.h -- the row tables of the kernels that take one (k_resample, the DSP kernels) on their way to the device: a ring of page-locked
// staging blocks and their device copies, a turn reused once the launches that read it have run.  DESIGN.md section 8 (N3).
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>

#include "common.h"

namespace ptts {

// When a turn of a row-table ring may be reused, without an event: a turn's upload carries a sequence number in front of its rows, a small
// copy queued behind the turn's launches hands the number back into page-locked memory, and the host waits for it there.  (The rings waited
// on lazily created events with hipEventSynchronize before; that call was seen to fail now and then with a stream-capture error -- "stream is
// capturing", "event last recorded in a capturing stream" -- on events that were never recorded into a capture.  This wait has no such state.)
struct RingAck {
    static constexpr int kRing = 8, kHead = 16;   // bytes in front of a turn's rows: the number, padded so that the rows stay 16-byte aligned
    uint64_t* back = nullptr;                     // page-locked [kRing]: what turn t last handed back
    uint64_t expect[kRing] = {};                  // ... and what its last launches will hand back (0: never used)
    uint64_t seq = 0;
    RingAck() = default;
    RingAck(const RingAck&) = delete;
    RingAck& operator=(const RingAck&) = delete;
    ~RingAck();
    void wait(int t);                                             // until turn t's last launches have run (throws PTTS_ENODEVICE after 60 s)
    // host_turn / dev_turn: the turn's blocks of kHead + row_bytes bytes; stamps the number, queues the upload of head and rows on s
    void upload(int t, char* host_turn, char* dev_turn, size_t row_bytes, hipStream_t s);
    void done(int t, const char* dev_turn, hipStream_t s);        // behind the turn's launches on s
};

// kRing turns of kRows rows, allocated on first use.  A launch sequence is stage(), the launches on the same stream, done().
// kTail: room behind a turn's rows for up to that many bytes the rows refer to by index (the DSP rows' equalisers), which travel in the
// same copy.
template <class Row, size_t kTail = 0>
struct RowRing {
    static constexpr int kRing = RingAck::kRing, kRows = 256;
    static constexpr size_t kTurnBytes = RingAck::kHead + ((sizeof(Row) * kRows + 15) & ~(size_t)15) + kTail;
    RowRing() = default;
    RowRing(const RowRing&) = delete;
    RowRing& operator=(const RowRing&) = delete;
    ~RowRing() {
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
    }
    // rows[0, n), n <= kRows, into the next turn (waits until that turn's last launches have run) and, on s, to the device: the device copy
    // tail[0, tail_bytes), tail_bytes <= kTail, goes behind the rows (16-byte aligned) in the same copy: *tail_dev receives its device copy
    const Row* stage(const Row* rows, int n, hipStream_t s, const void* tail = nullptr, size_t tail_bytes = 0, const void** tail_dev = nullptr) {
        if (!host) PTTS_HIP(hipHostMalloc((void**)&host, kTurnBytes * kRing, hipHostMallocDefault));
        if (!dev) PTTS_HIP(hipMalloc((void**)&dev, kTurnBytes * kRing));
        if (tail_bytes > kTail) throw Error(PTTS_EINVAL, "ptts-hip: a row table's tail does not fit its ring");
        turn = (turn + 1) % kRing;
        ack.wait(turn);
        char* h = host + (size_t)turn * kTurnBytes;
        size_t bytes = (size_t)n * sizeof(Row);
        std::memcpy(h + RingAck::kHead, rows, bytes);
        if (tail_bytes) {
            bytes = (bytes + 15) & ~(size_t)15;
            std::memcpy(h + RingAck::kHead + bytes, tail, tail_bytes);
            *tail_dev = dev_turn() + RingAck::kHead + bytes;
            bytes += tail_bytes;
        }
        ack.upload(turn, h, dev_turn(), bytes, s);
        return reinterpret_cast<const Row*>(dev_turn() + RingAck::kHead);
    }
    void done(hipStream_t s) { ack.done(turn, dev_turn(), s); }   // behind the launches that read the staged rows

private:
    char* dev_turn() const { return dev + (size_t)turn * kTurnBytes; }
    char *host = nullptr, *dev = nullptr;
    RingAck ack;
    int turn = kRing - 1;   // the turn staged last
};

}  // namespace ptts
