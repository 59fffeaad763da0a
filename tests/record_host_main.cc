// Stand-alone driver of gr_amps_amd/csrc/recc_record_host.h for tests/test_cpu_record_host.py: the sorted gather of a drain on a file of
// packed records, without a GPU, so that it can run under the sanitizers.
//   in : u64 n, u64 cap, n x PACKED_RECORD_BYTES packed records, n x PACKED_BURST_BYTES packed kept bursts
//   out: u64 returned, u64 truncated (as gather_sorted reports it: the drains' -ENOSPC), returned x amps_recc_burst_t, returned x AMPS_RECC_CAPTURE_SYMS kept symbols
#include <cstdio>
#include <vector>
#include "amps_recc.h"
#include "recc_record_host.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0, cap = 0;
    if (std::fread(&n, 8, 1, f) != 1 || std::fread(&cap, 8, 1, f) != 1) return 2;
    // exactly as large as the lists are: a read or write past either end is the sanitizer's to find
    std::vector<uint8_t> recs(n * amps::PACKED_RECORD_BYTES), kept(n * amps::PACKED_BURST_BYTES);
    if (std::fread(recs.data(), 1, recs.size(), f) != recs.size() || std::fread(kept.data(), 1, kept.size(), f) != kept.size()) return 2;
    std::fclose(f);
    std::vector<amps_recc_burst_t> out(cap);
    std::vector<uint8_t> bursts(cap * AMPS_RECC_CAPTURE_SYMS);
    std::vector<amps::RecordRef> refs;
    amps::record_refs_append(refs, recs.data(), n, amps::PACKED_RECORD_BYTES);
    bool truncated = false;
    const uint64_t k = amps::gather_sorted(refs, cap, &truncated, out.data(), recs.data(), kept.data(), bursts.data());
    const uint64_t overflow = truncated ? 1 : 0;
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(&k, 8, 1, f);
    std::fwrite(&overflow, 8, 1, f);
    if (k) {
        std::fwrite(out.data(), sizeof(amps_recc_burst_t), k, f);
        std::fwrite(bursts.data(), AMPS_RECC_CAPTURE_SYMS, k, f);
    }
    return std::fclose(f) == 0 ? 0 : 2;
}
