// recc_record_host.h -- a record's way from the capture kernel's packed form to the caller: layout, expansion, sort key and the sorted
// gather of a drain.  Plain host C++ (no HIP): tests/record_host_main.cc runs it under the sanitizers without a GPU.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "amps_recc.h"

namespace amps {

// one packed key (channel, position) for the capture queue and the host's sort: 2^44 samples per channel stream (2.8 years at 200 ksps), 2^20 channels
constexpr int CAPQ_POS_BITS = 44;
inline uint64_t record_key(uint32_t channel, uint64_t position) { return ((uint64_t)channel << CAPQ_POS_BITS) | (position & ((1ull << CAPQ_POS_BITS) - 1)); }

// ---- the record on its way to the host (round 5).  The capture kernels write their records straight into mapped, pinned HOST memory;
// 588 of a record's 728 bytes are the one-byte-per-bit arrays word_raw[7][48] and word_dec[7][36] the reference's own layout asks for
// (lib/recc_decode_impl.cc:92-95).  1664 records per push of the channel-major bench are 1.2 MB of 728-byte PCIe writes that the kernel
// cannot retire before they have crossed the link: 0.050 ms of "resolve + capture + decode" there was mostly that.  So the bits travel
// as bits -- PACKED_RECORD_BYTES = 216 instead of 728 -- and amps_recc_drain expands them while it gathers the sorted records into the
// caller's buffer anyway (expand_packed_record: one 8-byte table entry per packed byte).  Layout, in dwords:
//    0 .. 12   the record's first 52 bytes as they are (channel .. first_valid_rep)
//   13 .. 23   word_raw: bit 4 j + i of dword 13 + g = byte 32 g + 4 j + i of the array (bytes past the array's 336: don't care)
//   24 .. 31   word_dec likewise (252 bytes)
//   32 .. 53   the record's last 88 bytes as they are (a_F .. _pad4)
constexpr int PACKED_RECORD_BYTES = 216;
constexpr int PACKED_BURST_BYTES = (AMPS_RECC_CAPTURE_SYMS + 31) / 32 * 4;   // 424: the kept 3374-symbol blob, a bit per symbol (recc_resolve.hip.h: capture_store_wave)
constexpr int REC_RAW_OFF = 52, REC_DEC_OFF = 388, REC_TAIL_OFF = 640;
static_assert(offsetof(amps_recc_burst_t, word_raw) == REC_RAW_OFF && offsetof(amps_recc_burst_t, word_dec) == REC_DEC_OFF &&
              offsetof(amps_recc_burst_t, a_F) == REC_TAIL_OFF && sizeof(amps_recc_burst_t) - REC_TAIL_OFF == 88, "packed record layout");

// bits -> bytes, eight at a time: table entry v = the eight bytes (0 / 1) of the bits of v, bit i in byte i
inline const uint64_t *bit_bytes_lut()
{
    static const std::vector<uint64_t> lut = [] {
        std::vector<uint64_t> t(256);
        for (int v = 0; v < 256; v++) { uint64_t w = 0; for (int i = 0; i < 8; i++) w |= (uint64_t)((v >> i) & 1) << (8 * i); t[v] = w; }
        return t;
    }();
    return lut.data();
}
// a packed record (recc_decode.hip.h: decode_core_store_packed, 216 bytes) -> the ABI's amps_recc_burst_t: the two bit arrays back to
// one byte per bit
inline void expand_packed_record(amps_recc_burst_t *dst, const uint8_t *src)
{
    const uint64_t *lut = bit_bytes_lut();
    uint8_t *d = (uint8_t *)dst;
    std::memcpy(d, src, REC_RAW_OFF);
    const uint8_t *raw = src + 13 * 4, *dec = src + 24 * 4;
    for (int k = 0; k < (REC_DEC_OFF - REC_RAW_OFF) / 8; k++) std::memcpy(d + REC_RAW_OFF + 8 * k, &lut[raw[k]], 8);            // 42 x 8 = 336 bytes
    for (int k = 0; k < (REC_TAIL_OFF - REC_DEC_OFF + 7) / 8; k++) std::memcpy(d + REC_DEC_OFF + 8 * k, &lut[dec[k]], 8);        // 32 x 8: 4 bytes into the tail ...
    std::memcpy(d + REC_TAIL_OFF, src + 32 * 4, sizeof(amps_recc_burst_t) - REC_TAIL_OFF);                                       // ... which is written last
}

// the kept symbol blob: PACKED_BURST_BYTES of bits -> the 3374 bytes (values 0 / 1) gr::amps::recc publishes (lib/recc_impl.cc:126)
inline void expand_packed_burst(uint8_t *dst, const uint8_t *src)
{
    const uint64_t *lut = bit_bytes_lut();
    constexpr int FULL = AMPS_RECC_CAPTURE_SYMS / 8;                                                                             // 421 whole bytes of bits
    for (int k = 0; k < FULL; k++) std::memcpy(dst + 8 * k, &lut[src[k]], 8);
    for (int i = 8 * FULL; i < AMPS_RECC_CAPTURE_SYMS; i++) dst[i] = (uint8_t)((src[i >> 3] >> (i & 7)) & 1u);                    // the last six symbols
}

// The sorted gather of a drain: records in host memory, ordered by (channel, position) through compact 16-byte keys, then written
// once into the caller's buffer.  Channel and position sit in the first 16 bytes of a record in either form.
struct RecordRef { uint64_t key; const uint8_t *rec; };
inline void record_refs_append(std::vector<RecordRef> &refs, const void *recs, size_t n, size_t stride)
{
    const uint8_t *r = (const uint8_t *)recs;
    for (size_t i = 0; i < n; i++, r += stride) {
        uint32_t ch; uint64_t pos;
        std::memcpy(&ch, r + offsetof(amps_recc_burst_t, channel), 4);
        std::memcpy(&pos, r + offsetof(amps_recc_burst_t, position), 8);
        refs.push_back({ record_key(ch, pos), r });
    }
}
// Sorts refs and writes the first min(refs.size(), cap) records to out (if given): packed ones (`packed`: the list at `packed`,
// PACKED_RECORD_BYTES apart) expanded, others copied.  Of packed record i the kept blob is kept + i * PACKED_BURST_BYTES, expanded
// into bursts_out where both are given.  Returns the number of records that came back; *truncated says whether cap left some out
// (the -ENOSPC of either drain).
inline size_t gather_sorted(std::vector<RecordRef> &refs, size_t cap, bool *truncated, amps_recc_burst_t *out, const uint8_t *packed = nullptr,
                            const uint8_t *kept = nullptr, uint8_t *bursts_out = nullptr)
{
    *truncated = refs.size() > cap;
    std::sort(refs.begin(), refs.end(), [](const RecordRef &x, const RecordRef &y) { return x.key < y.key; });
    const size_t k = std::min(refs.size(), cap);
    for (size_t i = 0; i < k; i++) {
        if (out && packed) expand_packed_record(&out[i], refs[i].rec);
        else if (out) std::memcpy(&out[i], refs[i].rec, sizeof(amps_recc_burst_t));
        if (packed && kept && bursts_out)
            expand_packed_burst(bursts_out + i * AMPS_RECC_CAPTURE_SYMS, kept + (size_t)(refs[i].rec - packed) / PACKED_RECORD_BYTES * PACKED_BURST_BYTES);
    }
    return k;
}

// ---- reply generation: handle_response / handle_registration / handle_origination
// (lib/recc_decode_impl.cc:181-272) with the TX word builders of lib/amps_packet.cc:26-95.
// Host integer code, a few dozen byte stores per burst.
inline void put_bits(uint8_t *o, int n, uint64_t v) { for (int i = n - 1; i >= 0; i--) { o[i] = (uint8_t)(v & 1u); v >>= 1; } }
inline void word1(uint8_t *w, bool multi, unsigned dcc, uint64_t min1)
{
    w[0] = 0; w[1] = multi; w[2] = (dcc >> 1) & 1u; w[3] = dcc & 1u; put_bits(w + 4, 24, min1);
}
inline void word2_general(uint8_t *w, uint64_t min2, unsigned msg_type, unsigned ordq, unsigned order)
{
    w[0] = 1; w[1] = 0; w[2] = 1; w[3] = 1; put_bits(w + 4, 10, min2); w[14] = 0;
    put_bits(w + 15, 5, msg_type); put_bits(w + 20, 3, ordq); put_bits(w + 23, 5, order);
}
inline void word2_voice(uint8_t *w, unsigned scc, uint64_t min2, unsigned vmac, unsigned chan)
{
    w[0] = 1; w[1] = 0; w[2] = (scc >> 1) & 1u; w[3] = scc & 1u; put_bits(w + 4, 10, min2);
    put_bits(w + 14, 3, vmac); put_bits(w + 17, 11, chan);
}
inline void fvc_general(uint8_t *w, unsigned pscc, unsigned msg_type, unsigned ordq, unsigned order)
{
    std::memset(w, 0, 28);
    w[0] = 1; w[2] = 1; w[3] = 1; w[4] = (pscc >> 1) & 1u; w[5] = pscc & 1u;
    put_bits(w + 15, 5, msg_type); put_bits(w + 20, 3, ordq); put_bits(w + 23, 5, order);
}

inline int reply_words(const amps_recc_burst_t *b, amps_recc_reply_t *r)   // amps_recc_reply_words
{
    if (!b || !r) return -EINVAL;
    std::memset(r, 0, sizeof(*r));
    const unsigned DCC = 0, SCC = 1;     // GLOBAL_DCC_SHORT, GLOBAL_SCC (lib/amps_packet.h:13-14)
    const int STREAM_BOTH = 3;           // lib/amps_packet.h:33 (the A/B choice at :240-245 is overridden at :247)
    switch (b->msg_class) {
    case AMPS_MSG_REGISTRATION:          // :181-190 order confirmation = audit order 7
        r->has_focc = 1; r->focc_stream = STREAM_BOTH; r->focc_nwords = 2;
        word1(r->focc_word1, true, DCC, b->a_MIN1);
        word2_general(r->focc_word2, b->b_MIN2, 0, 0, 7);
        break;
    case AMPS_MSG_PAGE_RESPONSE:         // :195-222 voice channel 355, alert on the FVC
        r->has_focc = 1; r->focc_stream = STREAM_BOTH; r->focc_nwords = 2;
        word1(r->focc_word1, true, DCC, b->a_MIN1);
        word2_voice(r->focc_word2, SCC, b->b_MIN2, 0, 355);
        r->has_fvc = 1; r->fvc_count = 1; r->fvc_repeat = 35;
        fvc_general(r->fvc_word1, SCC, 0, 0, 1);
        r->has_mutes = 1; r->fvc_mute = 0; r->audio_mute = 1;
        break;
    case AMPS_MSG_ORIGINATION:           // :236-272 voice channel 356 (or reorder 9 for a leading '0')
        r->has_focc = 1; r->focc_stream = STREAM_BOTH; r->focc_nwords = 2;
        word1(r->focc_word1, true, DCC, b->a_MIN1);
        if (b->dialed[0] == '0') word2_general(r->focc_word2, b->b_MIN2, 0, 0, 9);
        else word2_voice(r->focc_word2, SCC, b->b_MIN2, 0, 356);
        r->has_mutes = 1; r->fvc_mute = 1; r->audio_mute = 0;
        r->has_command = 1;
        std::snprintf(r->command, sizeof(r->command), "page %.*s", 32, b->dialed);
        break;
    default: break;
    }
    return 0;
}

} // namespace amps
