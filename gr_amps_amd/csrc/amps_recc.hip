// amps_recc.hip -- C ABI implementation (include/amps_recc.h) over the gfx950 kernels.
// Host code only orchestrates: buffers, stream, launches, result copy-out.  There is no CPU
// compute path: every entry point that produces data launches HIP kernels, and handle creation
// fails with -ENODEV when no HIP device is usable.  The entry points here check their arguments and call the seams, each of which
// keeps its state and its host code in a header of its own (recc_*.hip.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "amps_recc.h"
#include "amps_recc_seizure.h"
#include "amps_recc_early.h"
#include "amps_recc_numerics.h"
#include "recc_timing.hip.h"
#include "recc_records.hip.h"
#include "recc_capture.hip.h"
#include "recc_symbols.hip.h"
#include "recc_channelizer.hip.h"
#include "recc_rccl.hip.h"
#include "recc_xlate.hip.h"
#include "recc_refchain.hip.h"

static_assert(sizeof(amps_recc_burst_t) == AMPS_RECC_BURST_BYTES, "record layout is part of the ABI");
static_assert(sizeof(amps_recc_burst_t) % 8 == 0, "records are copied as dwords");

using namespace amps;

// The handle: the configuration and one state per seam.  Every device and mapped-host allocation and every event belongs to one of
// the states, behind its owner (recc_devmem.hip.h).  Teardown (amps_recc_destroy): the bounded wait for the stream, collect_spans,
// rccl_destroy, then `delete`, which releases every seam's buffers and events -- members go in reverse order of declaration -- and
// the handle's own stream last, because it is declared first.  No buffer or event is named there: one added to a state cannot be
// left off a list.
struct amps_recc {
    Stream stream;                    // the handle's own, or cfg.stream borrowed
    amps_recc_cfg_t cfg{};
    int device = 0;
    uint32_t C = 0, sps = 0;
    int slicer = AMPS_SLICER_DEFAULT; // numeric spec of the slicer (AMPS_RECC_FLAG_SLICER_* select one explicitly)
    TimingState tm;
    RecordLists lists;                // where the capture seam's records go, and the split drain
    SeizureState seizures;            // seizure events (AMPS_RECC_FLAG_SEIZURE_EVENTS): what was reported, the event list
    EarlyState early;                 // early messages (AMPS_RECC_FLAG_EARLY_MESSAGES): how far each pending capture was looked at, the event list
    CaptureState cap;                 // trigger search, resolve, capture and decode behind the IQ seam and the wideband seam
    SymbolsState sym;
    BchScratch bch;                   // amps_bch_*
    ChannelizerState chz;             // wideband seam: the filter bank
    PowerRing power;                  // received power (AMPS_RECC_FLAG_CHANNEL_POWER or AMPS_RECC_FLAG_STREAM_POWER: one ring, filled by that seam's producer)
    AutocorrRing offset;              // carrier offset (AMPS_RECC_FLAG_STREAM_OFFSET or _OFFSET_UNIT: the lag-one autocorrelation sums of the IQ and translate seams)
    XlateState xl;                    // the translate stage in the form configured last (amps_recc_set_xlate / _set_xlate_shared)
    RefState ref;                     // reference-timing seam (G2 -> G3 -> G4 as the flow graph wires them; created on first use)
    RcclState rccl;                   // one band over several GPUs: amps_recc_rccl_init / amps_recc_push_wideband_bcast
};

namespace {

// Waits of the host on the handle's stream.  With a live communicator the handle's kernels may be queued behind a data collective
// whose peer has died: every such wait is bounded (rccl_wait / rccl_wait_event: on expiry the communicator is aborted, the collective
// returns and the stream drains) -- ADVICE r05: drain, destroy and reset used to sit in hipStreamSynchronize / hipEventSynchronize.
int sync_stream(amps_recc *h, hipStream_t s)
{
    if (h->rccl.comm && !h->rccl.dead) { if (int rc = rccl_wait(h->rccl, s)) return rc; return 0; }
    return hipStreamSynchronize(s) == hipSuccess ? 0 : -EIO;
}
int sync_event(amps_recc *h, hipEvent_t e)
{
    if (h->rccl.comm && !h->rccl.dead) { if (int rc = rccl_wait_event(h->rccl, e)) return rc; return 0; }
    return hipEventSynchronize(e) == hipSuccess ? 0 : -EIO;
}
// A communicator that died under work in flight leaves the stream state advanced over a block that never arrived: everything the
// handle would report from there on is void.  The data seams and the drains answer -ESTALE until amps_recc_reset.
#define STALE_CHECK(h) do { if ((h)->rccl.stale) return -ESTALE; } while (0)

// a channel-group handle owns its group's rows of the wideband seam only: its records are numbered through row2chan, which means
// nothing on the other seams
bool is_group_handle(const amps_recc *h) { return h->chz.enabled && h->chz.groups > 1; }

// what capture_run_iq and channelizer_run are handed: the power ring of a handle that keeps one
const PowerRing *power_of(const amps_recc *h) { return h->power.ring ? &h->power : nullptr; }
const AutocorrRing *offset_of(const amps_recc *h) { return h->offset.ring ? &h->offset : nullptr; }
const SeizureState *seizures_of(const amps_recc *h) { return h->seizures.enabled ? &h->seizures : nullptr; }
const EarlyState *early_of(const amps_recc *h) { return h->early.enabled ? &h->early : nullptr; }

int reset_state(amps_recc *h)
{
    hipStream_t s = h->stream.get();
    if (int rc = capture_reset(h->cap, s)) return rc;
    if (int rc = block_ring_reset(h->power, s)) return rc;
    if (int rc = block_ring_reset(h->offset, s)) return rc;
    if (int rc = records_reset(h->lists, s)) return rc;
    if (int rc = seizure_reset(h->seizures, s)) return rc;
    if (int rc = early_reset(h->early, s)) return rc;
    if (int rc = symbols_reset(h->sym, s)) return rc;
    if (int rc = channelizer_reset(h->chz, s)) return rc;
    if (int rc = xlate_reset(h->xl, s)) return rc;
    if (int rc = ref_reset(h->ref, s)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// The ring entry points (`ring`: h->power or h->offset, named by member so that a null handle is an argument error like any other).
// Errors in the order include/amps_recc.h states: -EINVAL for the arguments (args_ok), -ENOSYS without the ring, -ESTALE; a query by
// record then reports only for n = 0, is -E2BIG above 2^32 - 1 records, and finds a foreign channel (-EINVAL) before any wait.
int idle_stream(amps_recc *h) { HIP_TRY(hipSetDevice(h->device)); return sync_stream(h, h->stream.get()); }

template <class Ring> int ring_entry(amps_recc *h, Ring amps_recc::*ring, bool args_ok)
{
    if (!h || !args_ok) return -EINVAL;
    if (!(h->*ring).ring) return -ENOSYS;
    STALE_CHECK(h);
    return 0;
}

template <class Ring> int ring_channels(amps_recc *h, Ring amps_recc::*ring, uint64_t first, size_t n, float *out, size_t out_ld, uint32_t *rows, uint64_t *produced)
{
    if (int rc = ring_entry(h, ring, !n || (out && out_ld >= n))) return rc;
    if (int rc = idle_stream(h)) return rc;
    return block_ring_channels(h->*ring, h->cap.n_done, h->cap.origin, h->stream.get(), first, n, out, out_ld, rows, produced);
}

// res: one answer per record, for the caller to unpack; empty where nothing was asked
template <class Ring> int ring_bursts(amps_recc *h, Ring amps_recc::*ring, const amps_recc_burst_t *recs, size_t n, bool outs_ok, std::vector<typename Ring::result_t> &res)
{
    if (int rc = ring_entry(h, ring, !n || (recs && outs_ok))) return rc;
    if (n == 0) return 0;
    if (n > 0xffffffffull) return -E2BIG;
    return block_ring_bursts(h->*ring, h->cap.n_done, h->cap.origin, (uint32_t)AMPS_RECC_CAPTURE_SYMS * h->sps, h->stream.get(), [h] { return idle_stream(h); }, recs, n, res);
}

} // namespace

extern "C" {

int amps_recc_abi_version(void) { return AMPS_RECC_ABI_VERSION; }
int amps_recc_default_slicer(void) { return AMPS_SLICER_DEFAULT; }
uint32_t amps_recc_default_wideband_decim(void) { return chz_bank_of(CHZ_M)->default_decim; }
size_t amps_recc_burst_size(void) { return sizeof(amps_recc_burst_t); }

const char *amps_recc_strerror(int code)
{
    switch (-code) {
    case 0: return "ok";
    case EINVAL: return "invalid argument";
    case ENODEV: return "no usable HIP device (this library has no CPU fallback)";
    case ENOMEM: return "out of device or host memory";
    case EIO: return "HIP runtime error";
    case ENOSPC: return "result list overflowed max_bursts";
    case E2BIG: return "push larger than the configured capacity";
    case EOVERFLOW: return "trigger-hit list overflowed";
    case ENOSYS: return "seam not configured on this handle";
    case EBUSY: return "busy: a split drain is open, the stream has started, or the handle already has a communicator";
    case ETIMEDOUT: return "no answer from the other ranks within the RCCL timeout: communicator aborted";
    case ENOTCONN: return "the handle's communicator has been aborted";
    case ESTALE: return "the communicator died with collectives in flight: stream state and record lists are void until amps_recc_reset";
    case EREMOTEIO: return "another rank reported an error: no rank ran the collective";
    case ENODATA: return "end of stream: the root of the distributed push has no more samples";
    case ERANGE: return "samples not produced yet, or no longer held by the slicer bit ring";
    default: return "unknown error";
    }
}

int amps_recc_create(amps_recc_t **out, const amps_recc_cfg_t *cfg_in)
{
    if (!out || !cfg_in) return -EINVAL;
    *out = nullptr;
    if (cfg_in->struct_size != sizeof(amps_recc_cfg_t)) return -EINVAL;
    // everything that depends on the filter bank -- the wideband_* fields, a wideband handle's samples per symbol (decimation 0 = the
    // bank's default, samples per symbol 0 = what goes with it), the flags a bank has or lacks -- is admitted and filled in in one place
    amps_recc_cfg_t cfg_v;
    uint32_t rows = 0;                                                // the handle's: its channels, or its channel group's share of them
    if (int rc = chz_resolve_cfg(*cfg_in, &cfg_v, &rows)) return rc;
    const amps_recc_cfg_t *cfg = &cfg_v;
    if (cfg->n_channels < 1 || cfg->max_bursts < 1) return -EINVAL;
    // Two samples per symbol exist on the wideband seam only: the streaming kernel has the instantiation (recc_front_kernel<2, ...>),
    // reached by the two-kernel form of a bank that delivers 40 ksps per channel, and sps_supported refuses it to a handle of the IQ seam
    if (!cfg->wideband_channels && cfg->max_samples_per_push && !sps_supported(cfg->samples_per_symbol)) return -EINVAL;
    if (cfg->sync_tolerance > AMPS_RECC_MAX_SYNC_TOLERANCE) return -EINVAL;
    const uint32_t sl = cfg->flags & (AMPS_RECC_FLAG_SLICER_PRODUCT | AMPS_RECC_FLAG_SLICER_SINE | AMPS_RECC_FLAG_SLICER_ATAN | AMPS_RECC_FLAG_SLICER_EXACT);
    if (sl & (sl - 1)) return -EINVAL;                             // at most one slicer spec
    if (cfg->n_channels >= (1u << (64 - CAPQ_POS_BITS))) return -EINVAL;
    // power combines with the offset in either statistic, and a handle keeps one offset ring with one of them
    constexpr uint32_t OFFSET_FLAGS = AMPS_RECC_FLAG_STREAM_OFFSET | AMPS_RECC_FLAG_STREAM_OFFSET_UNIT;
    if ((cfg->flags & OFFSET_FLAGS) == OFFSET_FLAGS) return -EINVAL;
    if ((cfg->flags & AMPS_RECC_FLAG_SEIZURE_EVENTS) && !cfg->max_samples_per_push) return -EINVAL;   // the symbol seam has no trigger of its own to report
    if ((cfg->flags & AMPS_RECC_FLAG_EARLY_MESSAGES) && !cfg->max_samples_per_push) return -EINVAL;   // nor a capture that is still coming in
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -ENODEV;
    int dev = cfg->device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) return -ENODEV; }
    if (dev >= ndev) return -ENODEV;
    if (hipSetDevice(dev) != hipSuccess) return -ENODEV;

    // AMPS_RECC_TRACE_CREATE=1: the steps of this function to stderr (which HIP call a creation hangs or crawls in when many
    // processes share one device -- the 8-rank rehearsals of tests/test_gpu_bench_ranks.py)
    const bool trace = env_is("AMPS_RECC_TRACE_CREATE", [](const char *) { return true; });
    auto step = [&](const char *what) { if (trace) { std::fprintf(stderr, "amps_recc_create[%d]: %s\n", (int)getpid(), what); std::fflush(stderr); } };
    step("device set");
    amps_recc *h = new (std::nothrow) amps_recc();
    if (!h) return -ENOMEM;
    h->cfg = *cfg;
    h->device = dev;
    h->C = rows;
    h->sps = cfg->samples_per_symbol;
    h->slicer = (cfg->flags & AMPS_RECC_FLAG_SLICER_PRODUCT) ? AMPS_SLICER_PRODUCT
              : (cfg->flags & AMPS_RECC_FLAG_SLICER_SINE) ? AMPS_SLICER_SINE
              : (cfg->flags & AMPS_RECC_FLAG_SLICER_EXACT) ? AMPS_SLICER_EXACT
              : (cfg->flags & AMPS_RECC_FLAG_SLICER_ATAN) ? AMPS_SLICER_ATAN_BOXCAR : AMPS_SLICER_DEFAULT;
    timing_set_mode(h->tm, (cfg->flags & AMPS_RECC_FLAG_TIME_KERNELS) ? AMPS_RECC_TIMING_ALL : AMPS_RECC_TIMING_OFF);
    if (cfg->stream) h->stream.borrow((hipStream_t)cfg->stream);
    else if (h->stream.create()) { delete h; return -EIO; }
    step("stream created");
    int rc = symbols_create(h->sym, h->C, cfg->max_bursts);      // results + symbol seam (always present)
    step("symbol seam buffers allocated");
    if (!rc) rc = records_create(h->lists, cfg->max_bursts, (cfg->flags & AMPS_RECC_FLAG_KEEP_BURSTS) != 0);
    step("pinned record lists mapped");
    if (!rc && cfg->max_samples_per_push) rc = capture_create(h->cap, *cfg, h->C, h->slicer, cfg->wideband_channels != 0, dev);
    step("IQ seam buffers allocated");
    if (!rc && (cfg->flags & AMPS_RECC_FLAG_SEIZURE_EVENTS)) rc = seizure_create(h->seizures, h->C, cfg->max_bursts);
    if (!rc && (cfg->flags & AMPS_RECC_FLAG_EARLY_MESSAGES)) rc = early_create(h->early, h->C, cfg->max_bursts);
    if (!rc && (cfg->flags & AMPS_RECC_FLAG_STREAM_POWER)) rc = block_ring_create(h->power, PowerRule::BLOCK, h->C, h->cap.ring_words);
    if (!rc && (cfg->flags & OFFSET_FLAGS)) rc = block_ring_create(h->offset, PowerRule::BLOCK, h->C, h->cap.ring_words, (cfg->flags & AMPS_RECC_FLAG_STREAM_OFFSET_UNIT) != 0);
    if (!rc && cfg->wideband_channels) rc = channelizer_create(h->chz, *cfg);
    step("channelizer created");
    if (!rc && (cfg->flags & AMPS_RECC_FLAG_CHANNEL_POWER)) rc = block_ring_create(h->power, PowerRule::SNAPSHOT, h->chz.C, h->cap.ring_words, false, &h->chz.row2chan, cfg->n_channels);
    if (!rc) rc = reset_state(h);
    step("state reset");
    if (rc) { amps_recc_destroy(h); return rc; }
    *out = h;
    return 0;
}

void amps_recc_destroy(amps_recc_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)sync_stream(h, h->stream.get()); (void)hipStreamSynchronize(h->stream.get()); }   // bounded first: a dead peer must not hang the destructor
    collect_spans(h->tm);
    rccl_destroy(h->rccl);
    delete h;                                                // every seam's buffers and events, then the stream, if it is the handle's own (see struct amps_recc)
}

int amps_recc_reset(amps_recc_t *h)
{
    if (!h) return -EINVAL;
    HIP_TRY(hipSetDevice(h->device));
    (void)sync_stream(h, h->stream.get());          // bounded while a communicator lives (on expiry it is aborted and the stream drains)
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    collect_spans(h->tm);
    h->rccl.stale = false;                    // a fresh stream: whatever an aborted collective left behind is gone
    records_close(h->lists);
    return reset_state(h);
}

int amps_recc_push_symbols(amps_recc_t *h, const uint8_t *syms, size_t ld, int n, int mem,
                           uint8_t *bursts_out, uint32_t *burst_channel, size_t cap, size_t *nout)
{
    if (!h || !nout) return -EINVAL;
    *nout = 0;
    if (is_group_handle(h)) return -ENOSYS;
    if (n < 1) return 0;                                   // lib/recc_impl.cc:99-102
    if (n > AMPS_RECC_MAX_WORK_ITEMS) return -EINVAL;      // lib/recc_impl.cc:103
    if (!syms || ld < (size_t)n) return -EINVAL;
    HIP_TRY(hipSetDevice(h->device));
    return symbols_push(h->sym, h->tm, h->stream.get(), records_current(h->lists).status, syms, ld, n, mem, bursts_out, burst_channel, cap, nout);
}

int amps_recc_decode_bursts(amps_recc_t *h, const uint8_t *bursts, size_t nbursts, int mem,
                            const uint32_t *burst_channel, amps_recc_burst_t *out)
{
    if (!h || (!bursts && nbursts) || (!out && nbursts)) return -EINVAL;
    if (nbursts == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream.get();
    SymbolsState &y = h->sym;
    if (y.dec_out_dev.reserve(nbursts) || y.dec_in_dev.reserve(nbursts * AMPS_RECC_CAPTURE_SYMS) || y.dec_chan_dev.reserve(nbursts)) return -ENOMEM;
    const uint8_t *din = bursts;
    if (mem == AMPS_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(y.dec_in_dev.get(), bursts, nbursts * AMPS_RECC_CAPTURE_SYMS, hipMemcpyHostToDevice, s));
        din = y.dec_in_dev.get();
    }
    const uint32_t *dchan = nullptr;
    if (burst_channel) {
        HIP_TRY(hipMemcpyAsync(y.dec_chan_dev.get(), burst_channel, nbursts * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        dchan = y.dec_chan_dev.get();
    }
    {
        SpanGuard g(h->tm, s, false, T_DECODE);
        uint32_t grid = (uint32_t)std::min<size_t>(nbursts, 4096);
        hipLaunchKernelGGL(recc_decode_bursts_kernel, dim3(grid), dim3(64), 0, s, din, dchan, (uint32_t)nbursts, y.dec_out_dev.get(),
                           (h->cfg.flags & AMPS_RECC_FLAG_MAJORITY) ? 1u : 0u);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, y.dec_out_dev.get(), nbursts * sizeof(amps_recc_burst_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    collect_spans(h->tm);
    return 0;
}

int amps_recc_push_iq(amps_recc_t *h, const float *iq, size_t ld, size_t nsamp, int mem)
{
    if (!h) return -EINVAL;
    if (!h->cap.carry[0]) return -ENOSYS;
    if (is_group_handle(h)) return -ENOSYS;
    if (nsamp == 0) return 0;
    if (!iq || ld < nsamp) return -EINVAL;
    if (nsamp > h->cfg.max_samples_per_push) return -E2BIG;
    HIP_TRY(hipSetDevice(h->device));
    const float2 *d = (const float2 *)iq;
    uint64_t dld = ld;
    if (mem == AMPS_MEM_HOST) {
        if (int rc = h->cap.stage_iq.stage(d, ld, nsamp, h->C, (size_t)h->C * h->cfg.max_samples_per_push, &d, &dld)) return rc;
    }
    int rc = capture_run_iq(h->cap, h->lists, h->tm, h->stream.get(), d, dld, (uint32_t)nsamp, power_of(h), offset_of(h), seizures_of(h), early_of(h));
    if (!rc && mem == AMPS_MEM_HOST) rc = h->cap.stage_iq.arm(h->stream.get());
    return rc;
}

// the wideband seam for every sample format of the block (AMPS_RECC_SAMPLES_*): fc32, interleaved 16-bit I/Q
// (amps_recc_push_wideband_short) or 8-bit I/Q (amps_recc_push_wideband_as)
static int push_wideband_block(amps_recc_t *h, const void *iq, size_t nsamp, int mem, int format)
{
    if (!h || !chz_sample_bytes(format)) return -EINVAL;
    STALE_CHECK(h);
    if (!h->chz.enabled) return -ENOSYS;
    if (nsamp == 0) return 0;
    if (!iq) return -EINVAL;
    h->cap.origin_locked = true;
    HIP_TRY(hipSetDevice(h->device));
    // Fused form (default): filter bank + discriminator + boxcar + slicer in one kernel, then the bit-domain
    // correlator.  AMPS_RECC_FLAG_UNFUSED_WIDEBAND keeps the two-kernel form (channel-major intermediate in HBM), which is the only
    // form of the banks without a fused one.
    const bool fused = !(h->cfg.flags & AMPS_RECC_FLAG_UNFUSED_WIDEBAND) && h->chz.has(CHZ_HAS_FUSED);
    const float2 *chan_iq = nullptr;
    uint64_t ld = 0;
    uint32_t nout = 0;
    int rc;
    {
        SpanGuard g(h->tm, h->stream.get(), true, T_CHANNELIZER, nsamp);
        ChzRunIn in;
        in.iq = iq; in.nsamp = nsamp; in.mem = mem; in.format = format; in.fused = fused;
        in.gring = h->cap.gring.get(); in.ring_words = h->cap.ring_words; in.n_done = h->cap.n_done; in.slicer = h->slicer;
        in.power = power_of(h);
        in.after_main = SpanGuard::end_cb; in.after_ctx = &g;
        rc = channelizer_run(h->chz, in, h->stream.get(), &chan_iq, &ld, &nout);
    }
    if (rc) return rc;
    if (nout > h->cfg.max_samples_per_push) return -E2BIG;
    if (fused) return capture_run_bits(h->cap, h->lists, h->tm, h->stream.get(), nout, seizures_of(h), early_of(h));
    return capture_run_iq(h->cap, h->lists, h->tm, h->stream.get(), chan_iq, ld, nout, power_of(h), offset_of(h), seizures_of(h), early_of(h));   // (rings: CHZ_HAS_STREAM_RINGS only)
}

int amps_recc_push_wideband(amps_recc_t *h, const float *iq, size_t nsamp, int mem) { return push_wideband_block(h, iq, nsamp, mem, AMPS_RECC_SAMPLES_FC32); }
int amps_recc_push_wideband_short(amps_recc_t *h, const int16_t *iq, size_t nsamp, int mem) { return push_wideband_block(h, iq, nsamp, mem, AMPS_RECC_SAMPLES_SC16); }
int amps_recc_push_wideband_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem) { return push_wideband_block(h, iq, nsamp, mem, format); }

int amps_recc_rccl_unique_id(uint8_t *id)
{
    if (!id) return -EINVAL;
    RcclApi &api = rccl_api();
    if (!api.ok()) return -ENOSYS;
    RcclId uid;
    if (api.GetUniqueId(&uid) != 0) return -EIO;
    std::memcpy(id, uid.internal, sizeof(uid.internal));
    return 0;
}

int amps_recc_rccl_init(amps_recc_t *h, const uint8_t *id, int nranks, int rank)
{
    if (!h) return -EINVAL;
    if (!h->chz.has(CHZ_HAS_RCCL)) return -ENOSYS;              // one band over several GPUs is the 1024 bank's
    HIP_TRY(hipSetDevice(h->device));
    RcclLocal loc;
    loc.groups = h->cfg.wideband_groups >= 2 ? h->cfg.wideband_groups : 0;
    loc.group = h->cfg.wideband_group;
    // the largest block one push takes: max_samples_per_push frames of 512 samples (amps_recc_push_wideband: -E2BIG beyond)
    loc.cap_samples = (uint64_t)h->cfg.max_samples_per_push * (uint64_t)h->chz.D;
    loc.max_bursts = h->cfg.max_bursts;
    const int rc = rccl_init(h->rccl, id, nranks, rank, loc, sizeof(amps_recc_burst_t));
    if (rc == 0) h->rccl.timing = h->tm.mode != AMPS_RECC_TIMING_OFF;
    return rc;
}

int amps_recc_rccl_set_timeout(amps_recc_t *h, uint32_t milliseconds)
{
    if (!h || milliseconds == 0) return -EINVAL;
    h->rccl.timeout_ms = milliseconds;
    h->rccl.timeout_set = true;
    return 0;
}

int amps_recc_rccl_abort(amps_recc_t *h)
{
    if (!h) return -EINVAL;
    if (!h->rccl.comm) return h->rccl.dead ? 0 : -ENOSYS;
    HIP_TRY(hipSetDevice(h->device));
    rccl_kill(h->rccl);
    return 0;
}

int amps_recc_rccl_info(amps_recc_t *h, amps_recc_rccl_info_t *info)
{
    if (!h || !info || info->struct_size != sizeof(amps_recc_rccl_info_t)) return -EINVAL;
    RcclState &r = h->rccl;                                   // (no communicator yet: nranks = 0, the device fields are still filled)
    HIP_TRY(hipSetDevice(h->device));
    std::memset((char *)info + sizeof(info->struct_size), 0, sizeof(*info) - sizeof(info->struct_size));
    info->alive = r.comm ? 1 : 0;
    info->nranks = r.nranks; info->rank = r.rank;
    info->comm_nranks = -1; info->comm_rank = -1;
    // (librccl is loaded only for a handle that has, or had, a communicator: a single-GPU caller who asks for the device identity must
    // not pull a second copy of RCCL into a process that bundles its own -- ADVICE r05)
    const bool touched = r.comm != nullptr || r.dead;
    static RcclApi none;
    RcclApi &api = touched ? rccl_api() : none;
    if (r.comm && api.CommCount) { int v = -1; if (api.CommCount(r.comm, &v) == 0) info->comm_nranks = v; }
    if (r.comm && api.CommUserRank) { int v = -1; if (api.CommUserRank(r.comm, &v) == 0) info->comm_rank = v; }
    info->device = h->device;
    info->max_samples_per_push = r.cap_common;
    info->max_bursts_per_gather = r.mb_common;
    info->timeout_ms = r.timeout_ms;
    if (r.comm) for (int i = 0; i < 2; i++) rccl_harvest(r, i, true);
    info->collectives_timed = r.coll_count;
    info->collective_ms = r.coll_ms;
    info->collective_bytes = r.coll_count ? r.coll_bytes : 0;
    info->last_mode = r.last_mode;
    std::snprintf(info->library, sizeof(info->library), "%s", api.path);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess) {
        static_assert(sizeof(info->device_uuid) == sizeof(prop.uuid.bytes), "uuid");
        std::memcpy(info->device_uuid, prop.uuid.bytes, sizeof(info->device_uuid));
        info->pci_bus = prop.pciBusID; info->pci_device = prop.pciDeviceID; info->pci_domain = prop.pciDomainID;
    }
    return 0;
}

int amps_recc_push_wideband_dist(amps_recc_t *h, const float *iq, size_t nsamp, int mem, int root, int mode, size_t *npushed)
{
    if (npushed) *npushed = 0;
    if (!h) return -EINVAL;
    if (h->rccl.dead) return -ENOTCONN;
    if (!h->chz.enabled || h->chz.rs.enabled) return -ENOSYS;  // behind a resampler: the blocks RCCL carries are at the bank's rate, whatever the communicator
    if (!h->rccl.comm) return -ENOSYS;
    HIP_TRY(hipSetDevice(h->device));
    const float2 *blk = nullptr;
    int slot = 0;
    size_t n = 0;
    // (a missing block or nsamp = 0 at the root is the root's error -- both together its END OF STREAM, -ENODATA on every rank -- and
    // travels through the header: the other ranks learn of it)
    if (int rc = rccl_distribute(h->rccl, (const float2 *)iq, mem == AMPS_MEM_HOST, nsamp, root, mode, h->stream.get(), &blk, &slot, &n)) return rc;
    const int rc = amps_recc_push_wideband(h, (const float *)blk, n, AMPS_MEM_DEVICE);
    const int rc2 = rccl_block_consumed(h->rccl, slot, h->stream.get());
    if (npushed) *npushed = n;
    return rc ? rc : rc2;
}

int amps_recc_push_wideband_bcast(amps_recc_t *h, const float *iq, size_t nsamp, int mem, int root) { return amps_recc_push_wideband_dist(h, iq, nsamp, mem, root, AMPS_RECC_DIST_BROADCAST, nullptr); }

int amps_recc_drain_gather(amps_recc_t *h, amps_recc_burst_t *out, size_t cap, size_t *nout, int root)
{
    if (!h || !nout) return -EINVAL;
    *nout = 0;
    if (h->rccl.dead) return -ENOTCONN;
    if (!h->rccl.comm) return -ENOSYS;
    if (root < 0 || root >= h->rccl.nranks) return -EINVAL;      // (the same verdict on every rank: nobody is left alone in the collective)
    if (!out) cap = 0;
    HIP_TRY(hipSetDevice(h->device));
    // The handle's kernels wait for the data collectives: if a peer has gone, they never start, and an unbounded drain would sit behind
    // them for ever.  So the wait for the stream is bounded here (then the drain below finds it idle); on expiry the communicator is
    // aborted and the peers run into their own bound.
    if (int rc = rccl_wait(h->rccl, h->stream.get())) return rc;
    // this rank's own list first; whatever it returns, the rank then takes part in the collective (the others are waiting in it) and
    // tells them through the status word: bit 0 = its list overflowed, bit 1 = its drain failed
    std::vector<amps_recc_burst_t> mine(h->cfg.max_bursts);
    size_t n = 0;
    const int lrc = amps_recc_drain(h, mine.data(), mine.size(), &n);
    const uint32_t st = lrc == 0 ? 0u : lrc == -ENOSPC ? 1u : 2u;
    if (st & 2u) n = 0;
    std::vector<std::vector<uint8_t>> all;
    uint32_t st_or = 0;
    if (int rc = rccl_gather_records(h->rccl, mine.data(), (uint32_t)n, st, sizeof(amps_recc_burst_t), root, &all, &st_or)) return rc;
    bool truncated = false;
    if (h->rccl.rank == root) {
        std::vector<RecordRef> refs;
        for (const auto &v : all) record_refs_append(refs, v.data(), v.size() / sizeof(amps_recc_burst_t), sizeof(amps_recc_burst_t));
        *nout = gather_sorted(refs, cap, &truncated, out);         // a channel belongs to one rank: no ties
    }
    if (st_or & 2u) return (lrc && lrc != -ENOSPC) ? lrc : -EIO;
    return ((st_or & 1u) || truncated) ? -ENOSPC : 0;
}

// rows x n fc32 of a device block (row pitch ld) to the caller's host [rows][out_ld], then wait: the tail of the debug taps
static int copy_rows_out(amps_recc *h, const float2 *d, uint64_t ld, uint32_t n, float *out, size_t out_ld)
{
    if (n > out_ld) return -E2BIG;
    if (n)
        HIP_TRY(hipMemcpy2DAsync(out, out_ld * sizeof(float2), d, ld * sizeof(float2), (size_t)n * sizeof(float2), h->C,
                                 hipMemcpyDeviceToHost, h->stream.get()));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    return 0;
}

// design the channel filter and create the translate stage in one of its forms; center_hz is [n_channels]
static int xlate_configure(amps_recc *h, bool shared, uint32_t decim, double rate_hz, const double *center_hz, double gain, double cutoff, double width)
{
    // defaults = the flow graph's values (grc/recctest.grc:115-155, 889-937)
    if (gain == 0.0) gain = 3.0;
    if (cutoff == 0.0) cutoff = 10e3;
    if (width == 0.0) width = 4.5e3;
    // a filter the design can make (three taps or more, a cut-off within rate / 2), the form's decimations, the symbol rate the handle
    // was built for and the filter's length: xlate_admit, which the plan asks too.  -E2BIG is left to xlate_create, which checks the
    // centres first
    uint32_t ntaps = 0;
    if (xlate_admit(shared, decim, h->sps, rate_hz, cutoff, width, &ntaps) == -EINVAL) return -EINVAL;
    return xlate_create(h->xl, shared, h->C, decim, h->cfg.max_samples_per_push, rate_hz, center_hz,
                        xlate_design_taps(gain, rate_hz, cutoff, width), h->stream.get());
}

// run the translate stage on a block and hand its rows to the fused IQ seam
static int xlate_push(amps_recc *h, const void *iq, size_t ld, size_t nsamp, int format, int mem, const char *what)
{
    HIP_TRY(hipSetDevice(h->device));
    const float2 *f = nullptr;
    uint64_t fld = 0;
    uint32_t nout = 0;
    int rc;
    {
        SpanGuard g(h->tm, h->stream.get(), h->chz.enabled, T_XLATE, nsamp);
        rc = xlate_run(h->xl, iq, ld, nsamp, format, mem, h->stream.get(), &f, &fld, &nout);
    }
    if (rc) return rc;
    if (int rc2 = debug_sync(h->stream.get(), what)) return rc2;
    if (nout == 0) return 0;
    return capture_run_iq(h->cap, h->lists, h->tm, h->stream.get(), f, fld, nout, power_of(h), offset_of(h), seizures_of(h), early_of(h));
}

// test tap: run the translate stage alone and copy its rows out
static int xlate_debug(amps_recc *h, const void *iq, size_t ld, size_t nsamp, int format, int mem, float *out, size_t out_ld, size_t *nout)
{
    HIP_TRY(hipSetDevice(h->device));
    const float2 *f = nullptr;
    uint64_t fld = 0;
    uint32_t n = 0;
    int rc = xlate_run(h->xl, iq, ld, nsamp, format, mem, h->stream.get(), &f, &fld, &n);
    if (rc) return rc;
    *nout = n;
    return copy_rows_out(h, f, fld, n, out, out_ld);
}

int amps_recc_set_xlate(amps_recc_t *h, const amps_recc_xlate_cfg_t *x)
{
    if (!h || !x || x->struct_size != sizeof(amps_recc_xlate_cfg_t)) return -EINVAL;
    if (!h->cap.carry[0]) return -ENOSYS;                       // the IQ seam must be configured
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    if (x->decim == 0) { if (!h->xl.shared) xlate_destroy(h->xl); return 0; }   // removes the form this entry point configures
    const std::vector<double> centers(h->C, x->center_hz);  // every row uses the same centre
    return xlate_configure(h, false, x->decim, x->rate_hz, centers.data(), x->gain, x->cutoff_hz, x->width_hz);
}

// a sample format of the translate seams (AMPS_RECC_SAMPLES_*)
static bool xlate_format_ok(int format) { return xlate_sample_bytes(format) != 0; }

int amps_recc_push_raw_as(amps_recc_t *h, const void *iq, size_t ld, size_t nsamp, int format, int mem)
{
    if (!h || !xlate_format_ok(format)) return -EINVAL;
    if (!h->xl.enabled || h->xl.shared) return -ENOSYS;
    if (is_group_handle(h)) return -ENOSYS;
    if (nsamp == 0) return 0;
    if (!iq || ld < nsamp) return -EINVAL;
    return xlate_push(h, iq, ld, nsamp, format, mem, "xlate");
}
int amps_recc_push_raw(amps_recc_t *h, const float *iq, size_t ld, size_t nsamp, int mem) { return amps_recc_push_raw_as(h, iq, ld, nsamp, AMPS_RECC_SAMPLES_FC32, mem); }

int amps_recc_debug_xlate_as(amps_recc_t *h, const void *iq, size_t ld, size_t nsamp, int format, int mem, float *out, size_t out_ld, size_t *nout)
{
    if (!h || !iq || !out || !nout || ld < nsamp || !xlate_format_ok(format)) return -EINVAL;
    if (!h->xl.enabled || h->xl.shared) return -ENOSYS;
    return xlate_debug(h, iq, ld, nsamp, format, mem, out, out_ld, nout);
}
int amps_recc_debug_xlate(amps_recc_t *h, const float *iq, size_t ld, size_t nsamp, int mem, float *out, size_t out_ld, size_t *nout)
{
    return amps_recc_debug_xlate_as(h, iq, ld, nsamp, AMPS_RECC_SAMPLES_FC32, mem, out, out_ld, nout);
}

int amps_recc_set_xlate_shared(amps_recc_t *h, const amps_recc_xlate_shared_cfg_t *x)
{
    if (!h || !x || x->struct_size != sizeof(amps_recc_xlate_shared_cfg_t)) return -EINVAL;
    if (!h->cap.carry[0]) return -ENOSYS;                       // the IQ seam must be configured
    if (is_group_handle(h)) return -ENOSYS;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    if (x->decim == 0) { if (h->xl.shared && h->xl.L == 1) xlate_destroy(h->xl); return 0; }   // removes the form this entry point configures
    if (x->n_centers != h->C || !x->center_hz) return -EINVAL;
    return xlate_configure(h, true, x->decim, x->rate_hz, x->center_hz, x->gain, x->cutoff_hz, x->width_hz);
}

int amps_recc_xlate_shared_plan(double rate_hz, double width_hz, amps_recc_xlate_plan_t *out, size_t cap)
{
    if (width_hz == 0.0) width_hz = 4.5e3;                     // the default of xlate_configure
    if (!(rate_hz > 0.0) || std::isinf(rate_hz) || !(width_hz > 0.0) || (cap && !out)) return -EINVAL;
    int n = 0;
    for (uint32_t decim = 1; decim <= (uint32_t)XLW_MAX_D; decim++) {
        const double sps = std::nearbyint(rate_hz / decim / 20e3);
        if (!(sps >= 1.0 && sps <= 64.0) || !sps_supported((uint32_t)sps)) continue;
        uint32_t ntaps = 0;
        if (xlate_admit(true, decim, (uint32_t)sps, rate_hz, 10e3, width_hz, &ntaps)) continue;   // the default cut-off of xlate_configure
        if ((size_t)n < cap) out[n] = amps_recc_xlate_plan_t{ decim, (uint32_t)sps, ntaps, 0 };
        n++;
    }
    return n;
}

// both plan calls walk the bank table: the banks of 30 kHz bins in front of the banks of 10 kHz bins, a bank's default ratio first
int amps_recc_wideband_grid_plan(double rate_hz, amps_recc_wideband_grid_plan_t *out, size_t cap)
{
    if (!(rate_hz > 0.0) || std::isinf(rate_hz) || (cap && !out)) return -EINVAL;
    int n = 0;
    for (const ChzBank &b : CHZ_BANKS) {
        if (std::fabs(rate_hz - (double)b.sample_rate_hz()) > 0.5) continue;
        for (uint32_t D : b.decim) {
            if (!D) continue;
            if ((size_t)n < cap) out[n] = amps_recc_wideband_grid_plan_t{ b.M, D, b.samples_per_symbol(D), b.taps * b.M, b.bin_hz, b.stride, b.max_channels(), 0u };
            n++;
        }
    }
    return n;
}

// the banks of 30 kHz bins, a channel on every bin: what the call above answers for their rates (at most two ratios of one bank)
int amps_recc_wideband_plan(double rate_hz, amps_recc_wideband_plan_t *out, size_t cap)
{
    if (cap && !out) return -EINVAL;
    amps_recc_wideband_grid_plan_t g[2];
    int n = amps_recc_wideband_grid_plan(rate_hz, g, 2);
    if (n > 0 && g[0].channel_stride != 1u) n = 0;
    for (int i = 0; i < n; i++)
        if ((size_t)i < cap) out[i] = amps_recc_wideband_plan_t{ g[i].channels, g[i].decim, g[i].samples_per_symbol, g[i].taps };
    return n;
}

// the shared form behind a rational resampler: the same state, kernels chosen in xlate_run
int amps_recc_set_xlate_resampled(amps_recc_t *h, const amps_recc_xlate_resample_cfg_t *x)
{
    if (!h || !x || x->struct_size != sizeof(amps_recc_xlate_resample_cfg_t)) return -EINVAL;
    if (!h->cap.carry[0]) return -ENOSYS;                       // the IQ seam must be configured
    if (is_group_handle(h)) return -ENOSYS;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    if (x->decim == 0) { if (h->xl.shared && h->xl.L != 1) xlate_destroy(h->xl); return 0; }   // removes the form this entry point configures
    if (x->n_centers != h->C || !x->center_hz) return -EINVAL;
    // the defaults of xlate_configure; the prototype is the flow graph's filter at the up-sampled rate, its gain times interp for
    // the zero stuffing
    const double gain = x->gain == 0.0 ? 3.0 : x->gain, cutoff = x->cutoff_hz == 0.0 ? 10e3 : x->cutoff_hz, width = x->width_hz == 0.0 ? 4.5e3 : x->width_hz;
    uint32_t npp = 0;
    if (xlate_resample_admit(x->interp, x->decim, h->sps, x->rate_hz, cutoff, width, &npp) == -EINVAL) return -EINVAL;
    return xlate_create(h->xl, true, h->C, x->decim, h->cfg.max_samples_per_push, x->rate_hz, x->center_hz,
                        xlate_design_taps(gain * x->interp, x->interp * x->rate_hz, cutoff, width), h->stream.get(), x->interp);
}

int amps_recc_retune_xlate(amps_recc_t *h, const double *center_hz, size_t n)
{
    if (!h || !center_hz) return -EINVAL;
    STALE_CHECK(h);
    if (!h->xl.enabled) return -ENOSYS;
    HIP_TRY(hipSetDevice(h->device));
    return xlate_retune(h->xl, center_hz, n, h->stream.get());
}

// The tuner correction of the wideband seam: host state only.  The next launch of the bank carries the step by value, so nothing is
// written to the device, nothing is waited for, and the call may come between drain_begin and drain_end.
int amps_recc_set_wideband_shift(amps_recc_t *h, double shift_hz)
{
    if (!h) return -EINVAL;
    const ChzBank *b = h->chz.bank;                            // null without the wideband seam
    return wideband_shift_from(h->chz.has(CHZ_HAS_SHIFT), b ? b->M : 0u, b ? (double)b->bin_hz : 0.0, shift_hz, &h->chz.shift);
}

int amps_recc_wideband_shift(const amps_recc_t *h, double *shift_hz)
{
    if (!h || !shift_hz) return -EINVAL;
    if (!h->chz.has(CHZ_HAS_SHIFT)) return -ENOSYS;
    *shift_hz = h->chz.shift.hz;
    return 0;
}

// The resampler in front of the bank: admitted by wbr_admit, which the plan below asks too.  Nothing behind the resampler is touched.
int amps_recc_set_wideband_resample(amps_recc_t *h, const amps_recc_wideband_resample_cfg_t *r)
{
    if (!h || !r || r->struct_size != sizeof(amps_recc_wideband_resample_cfg_t)) return -EINVAL;
    ChannelizerState &z = h->chz;
    if (!z.enabled) return -ENOSYS;
    if (z.started) return -EBUSY;
    HIP_TRY(hipSetDevice(h->device));
    if (r->decim == 0) { z.rs = WbResampleState{}; return 0; }
    WbrFilter f;
    if (int rc = wbr_admit(*z.bank, r->interp, r->decim, r->rate_hz, r->cutoff_hz, r->width_hz, &f)) return rc;
    return wb_resample_create(z.rs, r->interp, r->decim, r->rate_hz, f,
                              xlate_design_taps((double)r->interp, r->interp * r->rate_hz, f.cutoff_hz, f.width_hz), h->stream.get());
}

int amps_recc_wideband_resample_plan(double rate_hz, amps_recc_wideband_resample_plan_t *out, size_t cap)
{
    if (!(rate_hz > 0.0) || std::isinf(rate_hz) || (cap && !out)) return -EINVAL;
    int n = 0;
    for (uint32_t interp = 1; interp <= WBR_MAX_LM; interp++)
        for (uint32_t decim = 1; decim <= WBR_MAX_LM; decim++)
            for (const ChzBank &b : CHZ_BANKS) {
                WbrFilter f;
                if (wbr_admit(b, interp, decim, rate_hz, 0.0, 0.0, &f)) continue;
                for (uint32_t D : b.decim) {
                    if (!D) continue;
                    if ((size_t)n < cap)
                        out[n] = amps_recc_wideband_resample_plan_t{ interp, decim, b.M, D, b.samples_per_symbol(D), f.npp, b.bin_hz, b.stride, (uint32_t)std::nearbyint(f.usable_hz), 0u };
                    n++;
                }
            }
    return n;
}

// test tap: the resampler alone, continuing its stream
int amps_recc_debug_wideband_resample(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem, float *out, size_t cap, size_t *nout)
{
    if (!h || !iq || !out || !nout || !chz_sample_bytes(format)) return -EINVAL;
    ChannelizerState &z = h->chz;
    if (!z.enabled || !z.rs.enabled) return -ENOSYS;
    if (wb_resample_count(z.rs, nsamp) > cap) return -E2BIG;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream.get();
    const void *d = iq;
    if (mem == AMPS_MEM_HOST) {                                // (never armed: the call ends with the stream idle)
        const size_t bytes = chz_sample_bytes(format) * nsamp;
        const uint8_t *staged = nullptr;
        uint64_t pitch = 0;
        if (int rc = z.stage.stage((const uint8_t *)iq, bytes, bytes, 1, bytes, &staged, &pitch)) return rc;
        d = staged;
    }
    uint32_t n = 0;
    if (int rc = wb_resample_run(z.rs, d, nsamp, format, s, &n)) return rc;
    z.started = true;
    if (n) HIP_TRY(hipMemcpyAsync(out, z.rs.out.get(), sizeof(float2) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *nout = n;
    return 0;
}

int amps_recc_xlate_resample_plan(double rate_hz, double width_hz, amps_recc_resample_plan_t *out, size_t cap)
{
    if (width_hz == 0.0) width_hz = 4.5e3;                     // the default of amps_recc_set_xlate_resampled
    if (!(rate_hz > 0.0) || std::isinf(rate_hz) || !(width_hz > 0.0) || (cap && !out)) return -EINVAL;
    int n = 0;
    for (uint32_t interp = XLR_MIN_L; interp <= (uint32_t)XLR_MAX_L; interp++)
        for (uint32_t decim = interp + 1; decim <= (uint32_t)XLR_MAX_M; decim++) {
            const double sps = std::nearbyint(rate_hz * interp / decim / 20e3);
            if (!(sps >= 1.0 && sps <= 64.0) || !sps_supported((uint32_t)sps)) continue;
            uint32_t npp = 0;
            if (xlate_resample_admit(interp, decim, (uint32_t)sps, rate_hz, 10e3, width_hz, &npp)) continue;   // the default cut-off
            if ((size_t)n < cap) out[n] = amps_recc_resample_plan_t{ interp, decim, (uint32_t)sps, npp };
            n++;
        }
    return n;
}

int amps_recc_push_raw_shared_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem)
{
    if (!h || !xlate_format_ok(format)) return -EINVAL;
    STALE_CHECK(h);
    if (!h->xl.enabled || !h->xl.shared) return -ENOSYS;
    if (is_group_handle(h)) return -ENOSYS;
    if (nsamp == 0) return 0;
    if (!iq) return -EINVAL;
    return xlate_push(h, iq, nsamp, nsamp, format, mem, "xlate_shared");
}
int amps_recc_push_raw_shared(amps_recc_t *h, const float *iq, size_t nsamp, int mem) { return amps_recc_push_raw_shared_as(h, iq, nsamp, AMPS_RECC_SAMPLES_FC32, mem); }

int amps_recc_debug_xlate_shared_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem, float *out, size_t out_ld, size_t *nout)
{
    if (!h || !iq || !out || !nout || !xlate_format_ok(format)) return -EINVAL;
    if (!h->xl.enabled || !h->xl.shared) return -ENOSYS;
    return xlate_debug(h, iq, nsamp, nsamp, format, mem, out, out_ld, nout);
}
int amps_recc_debug_xlate_shared(amps_recc_t *h, const float *iq, size_t nsamp, int mem, float *out, size_t out_ld, size_t *nout)
{
    return amps_recc_debug_xlate_shared_as(h, iq, nsamp, AMPS_RECC_SAMPLES_FC32, mem, out, out_ld, nout);
}

int amps_recc_refchain_symbols(amps_recc_t *h, const float *iq, size_t ld, size_t nsamp, int mem,
                               uint8_t *symbols_out, size_t sym_ld, uint32_t *nsym_out)
{
    if (!h || !symbols_out || !nsym_out || (nsamp && (!iq || ld < nsamp))) return -EINVAL;
    if (!h->cfg.max_samples_per_push) return -ENOSYS;
    if (h->sps != 10) return -EINVAL;                       // the flow graph's omega = 10 samples per symbol
    if (nsamp > h->cfg.max_samples_per_push) return -E2BIG;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream.get();
    if (!h->ref.ready) { if (int rc = ref_create(h->ref, h->C, h->cfg.max_samples_per_push, s)) return rc; }
    if (sym_ld < h->ref.sym_cap && sym_ld < nsamp / 9 + 16) return -EINVAL;
    const float2 *d = (const float2 *)iq;
    uint64_t dld = ld;
    if (mem == AMPS_MEM_HOST && nsamp) {   // (never armed: the call ends with the stream idle)
        if (int rc = h->ref.stage.stage(d, ld, nsamp, h->C, (size_t)h->C * h->cfg.max_samples_per_push, &d, &dld)) return rc;
    }
    if (int rc = ref_run(h->ref, d, dld, (uint32_t)nsamp, s)) return rc;
    HIP_TRY(hipMemcpyAsync(nsym_out, h->ref.nsym.get(), sizeof(uint32_t) * h->C, hipMemcpyDeviceToHost, s));
    const size_t w = std::min<size_t>(sym_ld, h->ref.sym_cap);
    HIP_TRY(hipMemcpy2DAsync(symbols_out, sym_ld, h->ref.syms.get(), h->ref.sym_cap, w, h->C, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int amps_recc_refchain_tables(amps_recc_t *h, float *atan258, float *mmse1032)
{
    if (!h || !atan258 || !mmse1032) return -EINVAL;
    if (!h->cfg.max_samples_per_push) return -ENOSYS;
    HIP_TRY(hipSetDevice(h->device));
    if (!h->ref.ready) { if (int rc = ref_create(h->ref, h->C, h->cfg.max_samples_per_push, h->stream.get())) return rc; }
    std::memcpy(atan258, h->ref.atan_host.data(), sizeof(float) * 258);
    std::memcpy(mmse1032, h->ref.mmse_host.data(), sizeof(float) * 129 * 8);
    return 0;
}

int amps_recc_wait_event(amps_recc_t *h, void *hip_event)
{
    if (!h || !hip_event) return -EINVAL;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamWaitEvent(h->stream.get(), (hipEvent_t)hip_event, 0));
    return 0;
}

int amps_recc_record_event(amps_recc_t *h, void *hip_event)
{
    if (!h || !hip_event) return -EINVAL;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventRecord((hipEvent_t)hip_event, h->stream.get()));
    return 0;
}

int amps_recc_drain_begin(amps_recc_t *h)
{
    if (!h) return -EINVAL;
    STALE_CHECK(h);
    if (h->lists.open_buf >= 0) return -EBUSY;
    HIP_TRY(hipSetDevice(h->device));
    return records_begin(h->lists, h->stream.get());
}

static int drain_end_impl(amps_recc_t *h, amps_recc_burst_t *out, uint8_t *bursts_out, size_t cap, size_t *nout)
{
    if (!h || !nout) return -EINVAL;
    *nout = 0;
    if (h->lists.open_buf < 0) return -EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) { records_close(h->lists); return -EIO; }
    // everything enqueued before drain_begin is done; later pushes may still run (bounded behind a collective)
    int rc = sync_event(h, h->lists.drain_event.get());
    if (!rc && h->rccl.stale) rc = -ESTALE;
    if (!rc) collect_spans(h->tm);
    rc = records_end(h->lists, rc, out, bursts_out, cap, nout);
    if (out && is_group_handle(h))                             // rows of a channel group -> channel numbers of the band selection
        for (size_t i = 0; i < *nout; i++) out[i].channel = out[i].channel < h->chz.row2chan.size() ? h->chz.row2chan[out[i].channel] : out[i].channel;
    return rc;
}
int amps_recc_drain_end(amps_recc_t *h, amps_recc_burst_t *out, size_t cap, size_t *nout) { return drain_end_impl(h, out, nullptr, cap, nout); }

// the whole drain in one call: begin and end
static int drain_whole(amps_recc_t *h, amps_recc_burst_t *out, uint8_t *bursts_out, size_t cap, size_t *nout)
{
    if (h->lists.open_buf >= 0) return -EBUSY;     // finish the split drain first
    if (int rc = amps_recc_drain_begin(h)) return rc;
    return drain_end_impl(h, out, bursts_out, cap, nout);
}

int amps_recc_drain_bursts(amps_recc_t *h, amps_recc_burst_t *out, uint8_t *bursts_out, size_t cap, size_t *nout)
{
    if (!h || !nout || !bursts_out) return -EINVAL;
    *nout = 0;
    if (!(h->cfg.flags & AMPS_RECC_FLAG_KEEP_BURSTS)) return -ENOSYS;
    return drain_whole(h, out, bursts_out, cap, nout);
}

int amps_recc_drain(amps_recc_t *h, amps_recc_burst_t *out, size_t cap, size_t *nout)
{
    if (!h || !nout) return -EINVAL;
    *nout = 0;
    return drain_whole(h, out, nullptr, cap, nout);
}

int amps_recc_drain_seizures(amps_recc_t *h, amps_recc_seizure_t *out, size_t cap, size_t *nout, size_t *nleft)
{
    if (!h || !nout || (!out && cap)) return -EINVAL;
    *nout = 0;
    if (nleft) *nleft = 0;
    if (!h->seizures.enabled) return -ENOSYS;
    STALE_CHECK(h);
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = sync_stream(h, h->stream.get())) return rc;
    const int rc = seizure_drain(h->seizures, h->stream.get(), out, cap, nout, nleft);
    if (is_group_handle(h))                                        // rows of a channel group -> channel numbers, as the records
        for (size_t i = 0; i < *nout; i++) out[i].channel = out[i].channel < h->chz.row2chan.size() ? h->chz.row2chan[out[i].channel] : out[i].channel;
    return rc;
}

int amps_recc_drain_early(amps_recc_t *h, amps_recc_early_t *out, size_t cap, size_t *nout, size_t *nleft)
{
    if (!h || !nout || (!out && cap)) return -EINVAL;
    *nout = 0;
    if (nleft) *nleft = 0;
    if (!h->early.enabled) return -ENOSYS;
    STALE_CHECK(h);
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = sync_stream(h, h->stream.get())) return rc;
    const int rc = early_drain(h->early, h->stream.get(), out, cap, nout, nleft);
    if (is_group_handle(h))                                        // rows of a channel group -> channel numbers, as the records
        for (size_t i = 0; i < *nout; i++) out[i].rec.channel = out[i].rec.channel < h->chz.row2chan.size() ? h->chz.row2chan[out[i].rec.channel] : out[i].rec.channel;
    return rc;
}

int amps_recc_debug_exact_slice(int form, int sps, const uint32_t *in, uint32_t *out)
{
    if (!in || !out) return -EINVAL;
    if (form == 1) {
        if (sps == 3) out[0] = exact_slice_word3(in[0], in[1], in[2], in[3], in[4], in[5], out[1], out[2]);
        else if (sps == 2) out[0] = exact_slice_word2(in[0], in[1], in[2], in[3], in[4], in[5], out[1], out[2]);
        else return -EINVAL;
        return 0;
    }
    if (form != 0) return -EINVAL;
    static const struct { int sps; uint32_t (*word)(uint32_t, uint32_t, uint32_t); } rates[] = {
        { 2, exact_slice_word<2> }, { 3, exact_slice_word<3> }, { 4, exact_slice_word<4> }, { 5, exact_slice_word<5> },
        { 6, exact_slice_word<6> }, { 8, exact_slice_word<8> }, { 10, exact_slice_word<10> }, { 12, exact_slice_word<12> } };
    for (const auto &r : rates) if (r.sps == sps) { out[0] = r.word(in[0], in[1], in[2]); return 0; }
    return -EINVAL;
}

int amps_recc_debug_demod(amps_recc_t *h, const float *iq, size_t nsamp, int mem, float *demod, float *soft, uint8_t *hard)
{
    if (!h || !iq) return -EINVAL;
    if (!h->cap.carry[0]) return -ENOSYS;
    if (nsamp == 0 || nsamp > h->cfg.max_samples_per_push) return -E2BIG;
    int rc = amps_recc_reset(h);
    if (rc) return rc;
    const size_t P = (nsamp / 64) * 64;
    if (h->cap.dbg_d.alloc(nsamp) || h->cap.dbg_S.alloc(nsamp)) { h->cap.dbg_d.reset(); h->cap.dbg_S.reset(); return -ENOMEM; }   // no tap may outlive the call
    // channel 0 only: replicate the single stream on every channel row is not needed, rows other than 0 read garbage-free zeros
    const float *src = iq;
    std::vector<float> tmp;
    if (h->C > 1) {
        if (mem != AMPS_MEM_HOST) { rc = -EINVAL; goto done; }
        tmp.assign((size_t)h->C * nsamp * 2, 0.f);
        std::memcpy(tmp.data(), iq, nsamp * 2 * sizeof(float));
        src = tmp.data();
    }
    rc = amps_recc_push_iq(h, src, nsamp, nsamp, mem);
    if (!rc && hipStreamSynchronize(h->stream.get()) != hipSuccess) rc = -EIO;
    if (!rc && P) {
        if (demod && hipMemcpy(demod, h->cap.dbg_d.get(), P * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = -EIO;
        if (soft && hipMemcpy(soft, h->cap.dbg_S.get(), P * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = -EIO;
        if (hard) {
            std::vector<uint64_t> ring(h->cap.ring_words);
            if (hipMemcpy(ring.data(), h->cap.gring.get(), sizeof(uint64_t) * h->cap.ring_words, hipMemcpyDeviceToHost) != hipSuccess) rc = -EIO;
            for (size_t i = 0; i < P; i++) hard[i] = (uint8_t)((ring[(i >> 6) & (h->cap.ring_words - 1)] >> (i & 63)) & 1ull);
        }
    }
done:
    h->cap.dbg_d.reset(); h->cap.dbg_S.reset();
    const int rc2 = amps_recc_reset(h);
    return rc ? rc : rc2;
}

int amps_recc_debug_channelize(amps_recc_t *h, const float *iq, size_t nsamp, int mem, float *out, size_t out_ld, size_t *nframes)
{
    return amps_recc_debug_channelize_as(h, iq, nsamp, AMPS_RECC_SAMPLES_FC32, mem, out, out_ld, nframes);
}

int amps_recc_debug_channelize_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem, float *out, size_t out_ld, size_t *nframes)
{
    if (!h || !iq || !out || !nframes || !chz_sample_bytes(format)) return -EINVAL;
    if (!h->chz.enabled) return -ENOSYS;
    HIP_TRY(hipSetDevice(h->device));
    const float2 *chan_iq = nullptr;
    uint64_t ld = 0;
    uint32_t nout = 0;
    ChzRunIn in;                                             // the unfused form: the channel-major block is the output
    in.iq = iq; in.nsamp = nsamp; in.mem = mem; in.format = format;
    int rc = channelizer_run(h->chz, in, h->stream.get(), &chan_iq, &ld, &nout);
    if (rc) return rc;
    *nframes = nout;
    return copy_rows_out(h, chan_iq, ld, nout, out, out_ld);
}

int amps_recc_debug_slicer_bits(amps_recc_t *h, uint64_t first, size_t n, uint8_t *out, size_t out_ld, uint32_t *rows, uint64_t *produced)
{
    if (!h || (n && (!out || out_ld < n))) return -EINVAL;
    if (!h->cap.gring) return -ENOSYS;
    STALE_CHECK(h);
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = sync_stream(h, h->stream.get())) return rc;
    // the slicers write ring words for [n_done, n_done + P) only, and n_done, origin and P are multiples of 64: after the wait the
    // ring holds the last R = 64 ring_words samples produced, never anything before the origin
    const uint64_t end = h->cap.n_done, span = 64ull * h->cap.ring_words;
    const uint64_t lo = std::max<uint64_t>(h->cap.origin, end > span ? end - span : 0);
    if (rows) *rows = h->C;
    if (produced) *produced = end;
    if (n == 0) return 0;
    if (first < lo || first > end || n > end - first) return -ERANGE;
    const uint64_t w0 = first >> 6, nw = ((first + n - 1) >> 6) - w0 + 1;      // <= ring_words
    const uint64_t s0 = w0 & (h->cap.ring_words - 1), n1 = std::min<uint64_t>(nw, h->cap.ring_words - s0);
    std::vector<uint64_t> words((size_t)h->C * nw);
    HIP_TRY(hipMemcpy2DAsync(words.data(), nw * 8, h->cap.gring.get() + s0, (size_t)h->cap.ring_words * 8, n1 * 8, h->C, hipMemcpyDeviceToHost, h->stream.get()));
    if (nw > n1)                                                                 // the range wraps round the ring's end
        HIP_TRY(hipMemcpy2DAsync(words.data() + n1, nw * 8, h->cap.gring.get(), (size_t)h->cap.ring_words * 8, (nw - n1) * 8, h->C, hipMemcpyDeviceToHost, h->stream.get()));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    for (size_t ch = 0; ch < h->C; ch++) {
        const uint64_t *w = words.data() + ch * nw;
        uint8_t *o = out + ch * out_ld;
        for (size_t i = 0; i < n; i++) {
            const uint64_t p = first + i;
            o[i] = (uint8_t)((w[(p >> 6) - w0] >> (p & 63)) & 1ull);
        }
    }
    return 0;
}

int amps_recc_channel_power(amps_recc_t *h, uint64_t first_snap, size_t n, float *out, size_t out_ld, uint32_t *rows, uint64_t *produced_snaps)
{
    return ring_channels(h, &amps_recc::power, first_snap, n, out, out_ld, rows, produced_snaps);
}

int amps_recc_burst_power(amps_recc_t *h, const amps_recc_burst_t *recs, size_t n, float *mean_power, uint32_t *n_snaps)
{
    std::vector<uint2> res;                                       // {mean as float bits, count}
    if (int rc = ring_bursts(h, &amps_recc::power, recs, n, mean_power && n_snaps, res)) return rc;
    for (size_t i = 0; i < res.size(); i++) { std::memcpy(&mean_power[i], &res[i].x, sizeof(float)); n_snaps[i] = res[i].y; }
    return 0;
}

uint32_t amps_recc_power_ring_snaps(const amps_recc_t *h) { return h && h->power.ring ? h->power.slots : 0u; }

int amps_recc_channel_autocorr(amps_recc_t *h, uint64_t first_block, size_t n, float *out, size_t out_ld, uint32_t *rows, uint64_t *produced_blocks)
{
    return ring_channels(h, &amps_recc::offset, first_block, n, out, out_ld, rows, produced_blocks);
}

int amps_recc_burst_autocorr(amps_recc_t *h, const amps_recc_burst_t *recs, size_t n, float *sum, uint32_t *n_blocks)
{
    std::vector<AutocorrBurstSum> res;
    if (int rc = ring_bursts(h, &amps_recc::offset, recs, n, sum && n_blocks, res)) return rc;
    for (size_t i = 0; i < res.size(); i++) { sum[2 * i] = res[i].re; sum[2 * i + 1] = res[i].im; n_blocks[i] = res[i].count; }
    return 0;
}

int amps_recc_burst_offset(amps_recc_t *h, const amps_recc_burst_t *recs, size_t n, float *offset_hz, uint32_t *n_blocks)
{
    if (!h || (n && (!recs || !offset_hz || !n_blocks))) return -EINVAL;
    if (!h->offset.ring) return -ENOSYS;
    std::vector<float> sum(2 * n);
    if (int rc = amps_recc_burst_autocorr(h, recs, n, sum.data(), n_blocks)) return rc;
    for (size_t i = 0; i < n; i++) offset_hz[i] = autocorr_offset_hz(sum[2 * i], sum[2 * i + 1], n_blocks[i], h->sps);
    return 0;
}

int amps_recc_set_origin(amps_recc_t *h, uint64_t first_sample)
{
    if (!h || (first_sample & 63u) || first_sample >= (1ull << CAPQ_POS_BITS)) return -EINVAL;
    if (!h->cap.carry[0]) return -ENOSYS;
    if (h->cap.n_done != 0 || h->cap.r_prev != 0 || h->cap.origin_locked) return -EBUSY;     // only on a fresh or reset handle
    h->cap.n_done = first_sample;
    h->cap.origin = first_sample;
    return 0;
}

int amps_recc_set_timing(amps_recc_t *h, int mode)
{
    if (!h || mode < AMPS_RECC_TIMING_OFF || mode > AMPS_RECC_TIMING_DOMINANT_SAMPLED) return -EINVAL;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    collect_spans(h->tm);
    timing_set_mode(h->tm, mode);
    h->rccl.timing = h->tm.mode != AMPS_RECC_TIMING_OFF;
    return 0;
}

int amps_recc_get_timing(amps_recc_t *h, amps_recc_timing_t *t, int reset)
{
    if (!h || !t) return -EINVAL;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    collect_spans(h->tm);
    std::memset(t, 0, sizeof(*t));
    t->struct_size = sizeof(*t);
    t->launches_front = h->tm.launches_front;
    t->ms_front = h->tm.ms[T_FRONT];
    t->ms_channelizer = h->tm.ms[T_CHANNELIZER];
    t->launches_channelizer = h->tm.launches_chz;
    t->ms_resolve = h->tm.ms[T_RESOLVE];
    t->ms_decode = h->tm.ms[T_DECODE];
    t->ms_carry = h->tm.ms[T_CARRY];
    t->ms_symbols = h->tm.ms[T_SYMBOLS];
    t->ms_xlate = h->tm.ms[T_XLATE];
    t->samples_front = h->tm.samples_front;
    if (reset) {
        for (double &m : h->tm.ms) m = 0;
        h->tm.launches_front = h->tm.launches_chz = 0;
        h->tm.samples_front = 0;
    }
    return 0;
}

// ---- BCH(63,51) shortened: batch encode / decode on the device (recc_decode.hip.h)
int amps_bch_encode_words(amps_recc_t *h, const uint8_t *msg, size_t nwords, int k, int mem, uint8_t *codewords)
{
    if (!h || k < 1 || k > 51 || (nwords && (!msg || !codewords))) return -EINVAL;
    if (nwords == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream.get();
    const uint8_t *din = nullptr;
    if (int rc = bch_stage_in(h->bch, s, msg, nwords * k, mem, &din)) return rc;
    const size_t nout = nwords * (size_t)(k + 12);
    if (int rc = bch_grow(h->bch.out, nout)) return rc;
    hipLaunchKernelGGL(bch_encode_words_kernel, dim3((unsigned)std::min<size_t>((nwords + 255) / 256, 4096)), dim3(256), 0, s, din, (uint32_t)nwords, k, h->bch.out.get());
    HIP_TRY(hipMemcpyAsync(codewords, h->bch.out.get(), nout, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int amps_bch_decode_words(amps_recc_t *h, const uint8_t *codewords, size_t nwords, int k, int mem, uint8_t *msg, uint8_t *valid, uint8_t *nerrors)
{
    if (!h || k < 1 || k > 51 || (nwords && (!codewords || !msg || !valid))) return -EINVAL;
    if (nwords == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream.get();
    BchScratch &b = h->bch;
    const uint8_t *din = nullptr;
    if (int rc = bch_stage_in(b, s, codewords, nwords * (size_t)(k + 12), mem, &din)) return rc;
    if (int rc = bch_grow(b.out, nwords * (size_t)k)) return rc;
    if (bch_grow(b.val, nwords) || bch_grow(b.err, nwords)) return -ENOMEM;
    hipLaunchKernelGGL(bch_decode_words_kernel, dim3((unsigned)std::min<size_t>((nwords + 255) / 256, 4096)), dim3(256), 0, s,
                       din, (uint32_t)nwords, k, b.out.get(), b.val.get(), b.err.get());
    HIP_TRY(hipMemcpyAsync(msg, b.out.get(), nwords * k, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(valid, b.val.get(), nwords, hipMemcpyDeviceToHost, s));
    if (nerrors) HIP_TRY(hipMemcpyAsync(nerrors, b.err.get(), nwords, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// reply generation (recc_record_host.h)
int amps_recc_reply_words(const amps_recc_burst_t *b, amps_recc_reply_t *r) { return reply_words(b, r); }

} // extern "C"
