// recc_records.hip.h -- the two record lists of a handle and the split drain.  Pushes append to the CURRENT list; drain_begin closes it
// (it is OPEN from then on) and makes the other one current; drain_end collects the open list.  The capture kernels write packed
// records into mapped, pinned host memory and their last workgroup publishes the list's header {count, status} there too, so a drain
// costs no copy on the stream.  A list's device-side words {slot allocator, status, ..} are cleared while it is NOT current, by
// whichever launch comes first (records_appending: the push's own housekeeping; records_begin: a memset).
#pragma once
#include "recc_devmem.hip.h"
#include "recc_record_host.h"

namespace amps {

constexpr size_t LIST_WORDS = 4;   // a record list's device-side words: {slot allocator, status, published count (recc_resolve.hip.h: publish_header), pad}
constexpr int HDR_STRIDE = 16;     // dwords between the two lists' host headers (one 64-byte line each: the CPU clears one while the GPU may write the other)

struct RecordLists {
    DevBuf<uint32_t> nrecords_buf[2];         // [LIST_WORDS] per list
    MappedBuf<amps_recc_burst_t> rec_buf[2];  // the capture kernel writes records here directly (PACKED_RECORD_BYTES each)
    MappedBuf<uint8_t> bsym_buf[2];           // AMPS_RECC_FLAG_KEEP_BURSTS: [max_bursts][PACKED_BURST_BYTES] (a bit per symbol; allocated for 3374 bytes each)
    MappedBuf<uint32_t> hdr;                  // {nrecords, status} per record list: written by the capture kernel's last workgroup
    Event drain_event;                        // behind everything enqueued before drain_begin
    uint32_t max_bursts = 0;
    bool list_clean[2] = { true, true };      // the device-side {nrecords, status} of the list are zero (or a launch that zeroes them is enqueued)
    int cur_buf = 0, open_buf = -1;
    bool open_untouched = false;      // no push has been enqueued since drain_begin: the open list's device counters are still there (header cross-check)
};

// What a kernel that appends to the current list takes into its arguments, all as the device sees it: the mapped records, the
// adjacent words {nrecords, status} (one 8-byte copy / memset serves both), the kept bursts (or null), the list's host header, and
// the capacity.
struct RecordListView { amps_recc_burst_t *records; uint32_t *nrecords, *status; uint8_t *burst_syms; uint32_t *hdr_host; uint32_t rec_cap; };
inline RecordListView records_current(const RecordLists &L)
{
    const int b = L.cur_buf;
    return { L.rec_buf[b].dev(), L.nrecords_buf[b].get(), L.nrecords_buf[b].get() + 1, L.bsym_buf[b].dev(), L.hdr.dev() + HDR_STRIDE * b, L.max_bursts };
}

// result records live in mapped, pinned host memory (zero copy: PACKED_RECORD_BYTES = 216 per burst over PCIe while the
// kernels run, expanded to the ABI's 728 by records_end)
inline int records_create(RecordLists &L, uint32_t max_bursts, bool keep_bursts)
{
    int rc = 0;
    L.max_bursts = max_bursts;
    for (int b = 0; b < 2; b++) {
        rc |= L.nrecords_buf[b].alloc(LIST_WORDS);
        rc |= L.rec_buf[b].alloc(max_bursts);
        if (keep_bursts) rc |= L.bsym_buf[b].alloc((size_t)max_bursts * AMPS_RECC_CAPTURE_SYMS);
    }
    rc |= L.hdr.alloc(2 * HDR_STRIDE);
    rc |= L.drain_event.create(hipEventDisableTiming);
    return rc ? -ENOMEM : 0;
}

// empties the host header of the open list and closes it: an error in a drain must not leave the handle answering -EBUSY for ever
inline void records_close(RecordLists &L)
{
    if (L.open_buf < 0) return;
    volatile uint32_t *hdr = L.hdr.host() + HDR_STRIDE * L.open_buf;
    hdr[0] = 0u; hdr[1] = 0u;
    L.open_buf = -1;
}

inline int records_reset(RecordLists &L, hipStream_t s)
{
    for (int b = 0; b < 2; b++) {
        HIP_TRY(hipMemsetAsync(L.nrecords_buf[b].get(), 0, LIST_WORDS * sizeof(uint32_t), s));
        L.list_clean[b] = true;
    }
    std::memset(L.hdr.host(), 0, 2 * HDR_STRIDE * sizeof(uint32_t));
    L.open_buf = -1; L.cur_buf = 0;
    return 0;
}

// A push is about to append to the current list.  Its streaming / bit-domain / resolve kernel also does the push's housekeeping
// (thread 0): it clears the {count, status} of the list that is NOT current if those are still dirty from its last use -- a list is
// only appended to while it is current, and a drain reads its header from host memory (published by the capture kernel), so the
// idle list's device counters are free to be cleared by any later launch.  Returns those words (the kernel's zero2), or null.
inline uint32_t *records_appending(RecordLists &L)
{
    L.open_untouched = false;               // this launch may clear the counters of the list a split drain has open
    const int idle = L.cur_buf ^ 1;
    uint32_t *zero2 = L.list_clean[idle] ? nullptr : L.nrecords_buf[idle].get();
    L.list_clean[idle] = true;
    L.list_clean[L.cur_buf] = false;        // the capture kernel of this push may append to the current list
    return zero2;
}

inline int records_begin(RecordLists &L, hipStream_t s)
{
    const int b = L.cur_buf;                // (nothing is open: the caller has answered -EBUSY otherwise)
    // the list's header is already on its way to host memory: the last capture workgroup of every push writes it
    HIP_TRY(hipEventRecord(L.drain_event.get(), s));
    L.open_buf = b;
    L.open_untouched = true;
    L.cur_buf = b ^ 1;                      // later pushes append to the other list
    if (!L.list_clean[b ^ 1]) {             // drained twice with no push in between: nobody has cleared it yet
        HIP_TRY(hipMemsetAsync(L.nrecords_buf[b ^ 1].get(), 0, LIST_WORDS * sizeof(uint32_t), s));
        L.list_clean[b ^ 1] = true;
    }
    return 0;
}

// Collects the open list.  The caller has waited for drain_event -- everything enqueued before records_begin is done, later pushes
// may still run -- and passes how that went: waited = 0, or the error to give up with.  Any error still CLOSES the split drain.
// AMPS_RECC_CHECK_HEADER=1 (the GPU test suite sets it): a drain that finds the stream idle behind it compares the header the
// capture kernel's last workgroup published to host memory with the list's device-side counters.  The publish orders three relaxed
// device atomics by their completion (recc_resolve.hip.h); this check is what would notice a compiler or architecture change
// breaking that.
inline int records_end(RecordLists &L, int waited, amps_recc_burst_t *out, uint8_t *bursts_out, size_t cap, size_t *nout)
{
    const int b = L.open_buf;
    auto fail = [&](int rc) { records_close(L); return rc; };
    if (waited) return fail(waited);
    volatile uint32_t *hdr = L.hdr.host() + HDR_STRIDE * b;
    uint32_t n = hdr[0];
    const uint32_t st = hdr[1];
    if (env_is("AMPS_RECC_CHECK_HEADER", env_one) && L.open_untouched) {
        uint32_t dev[2] = { 0u, 0u };
        if (hipMemcpy(dev, L.nrecords_buf[b].get(), sizeof(dev), hipMemcpyDeviceToHost) != hipSuccess) return fail(-EIO);
        if (dev[0] != n || dev[1] != st) {
            std::fprintf(stderr, "amps_recc: published list header {%u, %u} differs from the device counters {%u, %u}\n", n, st, dev[0], dev[1]);
            return fail(-EIO);
        }
    }
    records_close(L);                       // the header is empty until a capture kernel publishes into it again (the list is not current now)
    int rc = 0;
    if (st & 1u) rc = -EOVERFLOW;
    if ((st & (2u | 4u)) || n > L.max_bursts) { rc = -ENOSPC; }
    if (n > L.max_bursts) n = L.max_bursts;
    if (n) {
        // the records are already in host memory (written by the capture kernel, visible after the event above)
        const uint8_t *r = (const uint8_t *)L.rec_buf[b].host();
        std::vector<RecordRef> refs;
        refs.reserve(n);
        record_refs_append(refs, r, n, PACKED_RECORD_BYTES);
        bool truncated = false;
        *nout = gather_sorted(refs, cap, &truncated, out, r, L.bsym_buf[b].host(), bursts_out);
        if (truncated) rc = -ENOSPC;
    }
    // the list's device counters are cleared by the next push (records_appending) or by the next records_begin
    return rc;
}

} // namespace amps
