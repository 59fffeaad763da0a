"""ctypes binding of the C ABI (include/amps_recc.h) -- the only way Python reaches the HIP path.

There is deliberately no pure-Python / torch / numpy implementation of any entry point here: if
libamps_recc.so is missing or no HIP device is usable, calls raise (the library itself returns
-ENODEV from amps_recc_create).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMPS_RECC_LIB") or os.path.join(_HERE, "libamps_recc.so")  # env override: A/B builds only

CAPTURE = 3374
MAX_WORK_ITEMS = 61439
MEM_HOST, MEM_DEVICE = 0, 1
FLAG_TIME_KERNELS = 1
FLAG_MAJORITY = 2
FLAG_UNFUSED_WIDEBAND = 4
FLAG_SLICER_PRODUCT = 8
FLAG_SLICER_SINE = 16
FLAG_KEEP_BURSTS = 32
FLAG_SLICER_ATAN = 64
FLAG_SLICER_EXACT = 128
FLAG_FIXED_TIMING = 256
FLAG_CHANNEL_POWER = 512
FLAG_STREAM_POWER = 0x400                # received power on the IQ and translate seams (block means; channel_power: the wideband seam's snapshots)
FLAG_STREAM_OFFSET = 0x800               # carrier offset on the IQ and translate seams (lag-one autocorrelation sums per block)
FLAG_STREAM_OFFSET_UNIT = 0x1000         # the same ring and entry points with the unit-amplitude statistic (the one to use behind a channel filter)
FLAG_SEIZURE_EVENTS = 0x2000             # one event per seizure after the push in which its trigger was accepted (Recc.drain_seizures)
FLAG_EARLY_MESSAGES = 0x4000             # a message's announced words after the push in which the last of them arrived (Recc.drain_early)
SEIZURE_FLAG_DCC_COMPLETE = 1            # amps_recc_seizure_t.flags: dcc / dcc_bad were read (the 14 symbols behind the trigger were in)
POWER_STRIDE = 256                       # AMPS_RECC_POWER_STRIDE: channel-rate samples between two power snapshots / in one power block

# slicer names accepted by Recc(slicer=...): numeric spec of include/amps_recc_numerics.h -> cfg flag
_SLICER_FLAGS = {None: 0, "default": 0, "atan": FLAG_SLICER_ATAN, 0: FLAG_SLICER_ATAN, "A": FLAG_SLICER_ATAN,
                 "product": FLAG_SLICER_PRODUCT, 1: FLAG_SLICER_PRODUCT, "B": FLAG_SLICER_PRODUCT,
                 "sine": FLAG_SLICER_SINE, 2: FLAG_SLICER_SINE, "C": FLAG_SLICER_SINE,
                 "exact": FLAG_SLICER_EXACT, 3: FLAG_SLICER_EXACT, "D": FLAG_SLICER_EXACT}
SLICER_NAMES = ("atan", "product", "sine", "exact")      # indexed by AMPS_SLICER_*

MSG_CLASSES = ("invalid_word_a", "e_zero", "page_response", "registration", "origination", "bad_nawc", "unknown")

# mirrors amps_recc_burst_t; checked against amps_recc_burst_size() at load
BURST_DTYPE = np.dtype([
    ("channel", "<u4"), ("flags", "<u4"), ("position", "<u8"),
    ("dcc", "u1", (7,)), ("dcc_bad", "u1"),
    ("manch_bad", "<u2", (7,)), ("valid", "u1", (7,)), ("first_valid_rep", "u1", (7,)),
    ("word_raw", "u1", (7, 48)), ("word_dec", "u1", (7, 36)),
    ("a_F", "u1"), ("a_NAWC", "u1"), ("a_T", "u1"), ("a_S", "u1"), ("a_E", "u1"), ("a_ER", "u1"),
    ("a_SCM", "u1"), ("_pad0", "u1"), ("a_MIN1", "<u4"),
    ("b_F", "u1"), ("b_NAWC", "u1"), ("b_MSG_TYPE", "u1"), ("b_ORDQ", "u1"), ("b_ORDER", "u1"),
    ("b_LT", "u1"), ("b_EP", "u1"), ("b_SCM4", "u1"), ("b_MPCI", "u1"), ("b_SDCC1", "u1"),
    ("b_SDCC2", "u1"), ("_pad1", "u1"), ("b_MIN2", "<u2"), ("_pad2", "<u2"),
    ("esn", "<u4"), ("has_esn", "u1"), ("msg_class", "u1"), ("n_called_words", "u1"), ("_pad3", "u1"),
    ("min", "S12"), ("dialed", "S36"), ("_pad4", "<u4"),
], align=False)

# mirrors amps_recc_seizure_t of include/amps_recc_seizure.h (32 bytes)
SEIZURE_DTYPE = np.dtype([("channel", "<u4"), ("flags", "<u4"), ("position", "<u8"), ("dcc", "u1", (7,)), ("dcc_bad", "u1"),
                          ("found_at", "<u8")], align=False)

# mirrors amps_recc_early_t of include/amps_recc_early.h (744 bytes)
EARLY_DTYPE = np.dtype([("rec", BURST_DTYPE), ("found_at", "<u8"), ("n_words", "<u4"), ("_pad", "<u4")], align=False)


class Cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_channels", C.c_uint32), ("samples_per_symbol", C.c_uint32),
        ("max_samples_per_push", C.c_uint32), ("max_bursts", C.c_uint32), ("device", C.c_int32),
        ("flags", C.c_uint32), ("wideband_channels", C.c_uint32), ("wideband_decim", C.c_uint32),
        ("wideband_taps_per_branch", C.c_uint32), ("wideband_first_channel", C.c_uint32),
        ("sync_tolerance", C.c_uint32), ("wideband_groups", C.c_uint32), ("wideband_group", C.c_uint32), ("stream", C.c_void_p),
    ]


class Timing(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("launches_front", C.c_uint32), ("ms_front", C.c_double),
        ("ms_resolve", C.c_double), ("ms_decode", C.c_double), ("ms_carry", C.c_double),
        ("ms_symbols", C.c_double), ("samples_front", C.c_uint64),
        ("ms_channelizer", C.c_double), ("launches_channelizer", C.c_uint32), ("_pad", C.c_uint32),
        ("ms_xlate", C.c_double),
    ]


class XlateCfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("decim", C.c_uint32), ("rate_hz", C.c_double), ("center_hz", C.c_double),
        ("gain", C.c_double), ("cutoff_hz", C.c_double), ("width_hz", C.c_double),
    ]


class XlateSharedCfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("decim", C.c_uint32), ("n_centers", C.c_uint32), ("_pad", C.c_uint32),
        ("rate_hz", C.c_double), ("gain", C.c_double), ("cutoff_hz", C.c_double), ("width_hz", C.c_double),
        ("center_hz", C.POINTER(C.c_double)),
    ]


class XlatePlan(C.Structure):
    _fields_ = [("decim", C.c_uint32), ("samples_per_symbol", C.c_uint32), ("ntaps", C.c_uint32), ("_pad", C.c_uint32)]


class WidebandPlan(C.Structure):
    _fields_ = [("channels", C.c_uint32), ("decim", C.c_uint32), ("samples_per_symbol", C.c_uint32), ("taps", C.c_uint32)]


class WidebandGridPlan(C.Structure):
    _fields_ = [("channels", C.c_uint32), ("decim", C.c_uint32), ("samples_per_symbol", C.c_uint32), ("taps", C.c_uint32),
                ("bin_hz", C.c_uint32), ("channel_stride", C.c_uint32), ("max_channels", C.c_uint32), ("_pad", C.c_uint32)]


class XlateResampleCfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("interp", C.c_uint32), ("decim", C.c_uint32), ("n_centers", C.c_uint32), ("_pad", C.c_uint32),
        ("rate_hz", C.c_double), ("gain", C.c_double), ("cutoff_hz", C.c_double), ("width_hz", C.c_double),
        ("center_hz", C.POINTER(C.c_double)),
    ]


class ResamplePlan(C.Structure):
    _fields_ = [("interp", C.c_uint32), ("decim", C.c_uint32), ("samples_per_symbol", C.c_uint32), ("ntaps_per_phase", C.c_uint32)]


class WidebandResampleCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("interp", C.c_uint32), ("decim", C.c_uint32), ("_pad", C.c_uint32),
                ("rate_hz", C.c_double), ("cutoff_hz", C.c_double), ("width_hz", C.c_double)]


class WidebandResamplePlan(C.Structure):
    _fields_ = [("interp", C.c_uint32), ("decim", C.c_uint32), ("channels", C.c_uint32), ("bank_decim", C.c_uint32),
                ("samples_per_symbol", C.c_uint32), ("ntaps_per_phase", C.c_uint32), ("bin_hz", C.c_uint32), ("channel_stride", C.c_uint32),
                ("usable_hz", C.c_uint32), ("_pad", C.c_uint32)]


class RcclInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("alive", C.c_int32), ("nranks", C.c_int32), ("rank", C.c_int32),
        ("comm_nranks", C.c_int32), ("comm_rank", C.c_int32), ("device", C.c_int32),
        ("pci_domain", C.c_int32), ("pci_bus", C.c_int32), ("pci_device", C.c_int32),
        ("device_uuid", C.c_uint8 * 16), ("max_samples_per_push", C.c_uint64), ("max_bursts_per_gather", C.c_uint32),
        ("timeout_ms", C.c_uint32), ("collectives_timed", C.c_uint64), ("collective_ms", C.c_double),
        ("collective_bytes", C.c_uint64), ("last_mode", C.c_int32), ("_pad", C.c_int32), ("library", C.c_char * 96),
    ]


class Reply(C.Structure):
    _fields_ = [
        ("has_focc", C.c_uint8), ("focc_stream", C.c_int32), ("focc_nwords", C.c_int32),
        ("focc_word1", C.c_uint8 * 28), ("focc_word2", C.c_uint8 * 28),
        ("has_fvc", C.c_uint8), ("fvc_count", C.c_int32), ("fvc_word1", C.c_uint8 * 28),
        ("fvc_repeat", C.c_uint64),
        ("has_mutes", C.c_uint8), ("fvc_mute", C.c_uint8), ("audio_mute", C.c_uint8),
        ("has_command", C.c_uint8), ("command", C.c_char * 48),
    ]


def _prototypes():
    """Every entry point of include/amps_recc.h, in the header's order: name -> (restype, argtypes).  A new entry point is one row
    here and one method body below; tests/test_cpu_capi_prototypes.py holds the rows to the header's declarations."""
    vp, i, sz, u32, u64, dbl = C.c_void_p, C.c_int, C.c_size_t, C.c_uint32, C.c_uint64, C.c_double
    psz, pu32, pu64, pdbl = C.POINTER(sz), C.POINTER(u32), C.POINTER(u64), C.POINTER(dbl)
    ring_rows = [vp, u64, sz, vp, sz, pu32, pu64]          # (h, first, n, out, out_ld, &rows, &produced)
    ring_bursts = [vp, vp, sz, vp, vp]                     # (h, records, n, value out, count out)
    return {
        "amps_recc_abi_version": (i, []),
        "amps_recc_default_slicer": (i, []),
        "amps_recc_default_wideband_decim": (u32, []),
        "amps_recc_strerror": (C.c_char_p, [i]),
        "amps_recc_burst_size": (sz, []),
        "amps_recc_create": (i, [C.POINTER(vp), C.POINTER(Cfg)]),
        "amps_recc_destroy": (None, [vp]),
        "amps_recc_reset": (i, [vp]),
        "amps_recc_set_origin": (i, [vp, u64]),
        "amps_recc_push_symbols": (i, [vp, vp, sz, i, i, vp, vp, sz, psz]),
        "amps_recc_decode_bursts": (i, [vp, vp, sz, i, vp, vp]),
        "amps_recc_push_iq": (i, [vp, vp, sz, sz, i]),
        "amps_recc_push_wideband": (i, [vp, vp, sz, i]),
        "amps_recc_push_wideband_short": (i, [vp, vp, sz, i]),
        "amps_recc_set_xlate": (i, [vp, C.POINTER(XlateCfg)]),
        "amps_recc_push_raw": (i, [vp, vp, sz, sz, i]),
        "amps_recc_debug_xlate": (i, [vp, vp, sz, sz, i, vp, sz, psz]),
        "amps_recc_set_xlate_shared": (i, [vp, C.POINTER(XlateSharedCfg)]),
        "amps_recc_xlate_shared_plan": (i, [dbl, dbl, C.POINTER(XlatePlan), sz]),
        "amps_recc_wideband_plan": (i, [dbl, C.POINTER(WidebandPlan), sz]),
        "amps_recc_wideband_grid_plan": (i, [dbl, C.POINTER(WidebandGridPlan), sz]),
        "amps_recc_push_raw_shared": (i, [vp, vp, sz, i]),
        "amps_recc_debug_xlate_shared": (i, [vp, vp, sz, i, vp, sz, psz]),
        "amps_recc_set_xlate_resampled": (i, [vp, C.POINTER(XlateResampleCfg)]),
        "amps_recc_xlate_resample_plan": (i, [dbl, dbl, C.POINTER(ResamplePlan), sz]),
        "amps_recc_push_raw_shared_as": (i, [vp, vp, sz, i, i]),
        "amps_recc_push_raw_as": (i, [vp, vp, sz, sz, i, i]),
        "amps_recc_debug_xlate_shared_as": (i, [vp, vp, sz, i, i, vp, sz, psz]),
        "amps_recc_debug_xlate_as": (i, [vp, vp, sz, sz, i, i, vp, sz, psz]),
        "amps_recc_push_wideband_as": (i, [vp, vp, sz, i, i]),
        "amps_recc_debug_channelize_as": (i, [vp, vp, sz, i, i, vp, sz, psz]),
        "amps_recc_set_wideband_shift": (i, [vp, dbl]),
        "amps_recc_wideband_shift": (i, [vp, pdbl]),
        "amps_recc_set_wideband_resample": (i, [vp, C.POINTER(WidebandResampleCfg)]),
        "amps_recc_wideband_resample_plan": (i, [dbl, C.POINTER(WidebandResamplePlan), sz]),
        "amps_recc_debug_wideband_resample": (i, [vp, vp, sz, i, i, vp, sz, psz]),
        "amps_recc_retune_xlate": (i, [vp, pdbl, sz]),
        "amps_recc_refchain_symbols": (i, [vp, vp, sz, sz, i, vp, sz, vp]),
        "amps_recc_refchain_tables": (i, [vp, vp, vp]),
        "amps_recc_wait_event": (i, [vp, vp]),
        "amps_recc_record_event": (i, [vp, vp]),
        "amps_recc_drain": (i, [vp, vp, sz, psz]),
        "amps_recc_drain_begin": (i, [vp]),
        "amps_recc_drain_end": (i, [vp, vp, sz, psz]),
        "amps_recc_drain_bursts": (i, [vp, vp, vp, sz, psz]),
        "amps_recc_debug_demod": (i, [vp, vp, sz, i, vp, vp, vp]),
        "amps_recc_debug_slicer_bits": (i, ring_rows),
        "amps_recc_channel_power": (i, ring_rows),
        "amps_recc_burst_power": (i, ring_bursts),
        "amps_recc_power_ring_snaps": (u32, [vp]),
        "amps_recc_channel_autocorr": (i, ring_rows),
        "amps_recc_burst_autocorr": (i, ring_bursts),
        "amps_recc_burst_offset": (i, ring_bursts),
        "amps_recc_rccl_unique_id": (i, [vp]),
        "amps_recc_rccl_init": (i, [vp, vp, i, i]),
        "amps_recc_rccl_set_timeout": (i, [vp, u32]),
        "amps_recc_rccl_abort": (i, [vp]),
        "amps_recc_push_wideband_dist": (i, [vp, vp, sz, i, i, i, psz]),
        "amps_recc_push_wideband_bcast": (i, [vp, vp, sz, i, i]),
        "amps_recc_drain_gather": (i, [vp, vp, sz, psz, i]),
        "amps_recc_rccl_info": (i, [vp, C.POINTER(RcclInfo)]),
        "amps_recc_debug_exact_slice": (i, [i, i, pu32, pu32]),
        "amps_recc_debug_channelize": (i, [vp, vp, sz, i, vp, sz, psz]),
        "amps_recc_get_timing": (i, [vp, C.POINTER(Timing), i]),
        "amps_recc_set_timing": (i, [vp, i]),
        "amps_recc_reply_words": (i, [vp, C.POINTER(Reply)]),
        "amps_bch_encode_words": (i, [vp, vp, sz, i, i, vp]),
        "amps_bch_decode_words": (i, [vp, vp, sz, i, i, vp, vp, vp]),
    }


PROTOTYPES = _prototypes()
EXPORTS = tuple(PROTOTYPES)
# The entry points of the extension headers, in the same form: include/amps_recc_seizure.h (seizure events).  load() sets them up with
# the table above; tests/test_cpu_seizure_events.py holds the rows to that header's declarations.
EXTENSION_PROTOTYPES = {
    "amps_recc_drain_seizures": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
}
EXTENSION_EXPORTS = tuple(EXTENSION_PROTOTYPES)
# include/amps_recc_early.h (early messages), a table of its own: tests/test_cpu_early_messages.py holds the rows to that header
EARLY_PROTOTYPES = {
    "amps_recc_drain_early": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
}
EARLY_EXPORTS = tuple(EARLY_PROTOTYPES)
GRID10_CHANNELS = (2500, 2000, 1000, 500)   # branches of the wideband seam's banks of 10 kHz bins: 25, 20, 10 and 5 Msps
DIST_BROADCAST, DIST_SCATTER_ALLGATHER = 0, 1
# sample formats of the translate seams' _as entry points (AMPS_RECC_SAMPLES_*): the element dtype of a block, two per sample
SAMPLES_FC32, SAMPLES_SC16, SAMPLES_SC8, SAMPLES_CU8 = 0, 1, 2, 3
SAMPLE_DTYPES = {SAMPLES_FC32: np.dtype(np.float32), SAMPLES_SC16: np.dtype(np.int16), SAMPLES_SC8: np.dtype(np.int8), SAMPLES_CU8: np.dtype(np.uint8)}
DIST_MODES = {"broadcast": DIST_BROADCAST, "scatter_allgather": DIST_SCATTER_ALLGATHER, 0: 0, 1: 1}

_lib = None


class AmpsError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = load().amps_recc_strerror(code).decode() if _lib is not None else "library not loaded"
        super().__init__(f"{where}: {msg} ({code})")


def load():
    """dlopen the C-ABI library.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built -- run `python -c 'import __graft_entry__ as g; g.build()'`; "
                          "there is no CPU fallback for the RECC path")
    L = C.CDLL(LIB_PATH)
    missing = []
    for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(EXTENSION_PROTOTYPES.items()) + list(EARLY_PROTOTYPES.items()):
        fn = getattr(L, name, None)
        if fn is None:
            missing.append(name)
            continue
        fn.restype = restype
        fn.argtypes = argtypes
    # the tree's own library has every entry point; an A/B library of another revision (AMPS_RECC_LIB) may lack some, and calling
    # one of those is an AttributeError
    if missing and not os.environ.get("AMPS_RECC_LIB"):
        raise ImportError(f"{LIB_PATH} lacks {', '.join(missing)} -- rebuild it")
    if L.amps_recc_burst_size() != BURST_DTYPE.itemsize:
        raise ImportError("amps_recc_burst_t layout mismatch between binding and library")
    _lib = L
    return L


def _call(name, *args):
    """entry point `name` of the library; a non-zero result is an AmpsError that carries the name"""
    rc = getattr(load(), name)(*args)
    if rc:
        raise AmpsError(rc, name)


def _plan(name, struct, *rate):
    """a *_plan entry point: ask how many entries (rate..., NULL, 0) answers, fetch them, one tuple of the struct's fields each"""
    fn = getattr(load(), name)
    n = fn(*rate, None, 0)
    if n < 0:
        raise AmpsError(n, name)
    out = (struct * max(n, 1))()
    n = fn(*rate, out, n)
    fields = [f for f, _ in struct._fields_ if f != "_pad"]
    return [tuple(int(getattr(p, f)) for f in fields) for p in out[:n]]


def _hostptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _fc32_rows(iq, rows):
    """fc32 rows [rows][ld] -> (block, ld): a numpy array is cast to complex64 and reshaped, a tensor is taken as it is"""
    if isinstance(iq, np.ndarray):
        iq = np.ascontiguousarray(iq, np.complex64).reshape(rows, -1)
    return iq, iq.shape[1]


def _fc32_row(iq):
    """one fc32 row -> (block, n): a numpy array is cast to complex64 and flattened, a tensor is taken as it is"""
    if isinstance(iq, np.ndarray):
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
    return iq, iq.shape[0]


def _as_ptr(x, sync_torch=True):
    """numpy array -> (pointer, MEM_HOST, keepalive); torch CUDA tensor -> (pointer, MEM_DEVICE, keepalive).
    The library launches on its own non-blocking stream, which is not ordered against torch's: a device tensor is pushed
    only after the torch stream that produced it has drained (a pageable H2D copy or a generator kernel may still be in
    flight when .to() / randn() return).  Callers that order the streams themselves (Recc.wait_torch) pass sync_torch=False."""
    if isinstance(x, np.ndarray):
        return _hostptr(x), MEM_HOST, x
    if hasattr(x, "data_ptr"):
        if x.is_cuda:
            if sync_torch:
                import torch
                torch.cuda.current_stream(x.device).synchronize()
            return C.c_void_p(x.data_ptr()), MEM_DEVICE, x
        a = x.numpy()
        return _hostptr(a), MEM_HOST, a
    raise TypeError(type(x))


def convert_samples(a, format):
    """The DEFINITION of the translate seams' sample formats (include/amps_recc.h, AMPS_RECC_SAMPLES_*), in numpy: a block of
    `format`'s dtype, shaped [..., n, 2] or [..., 2n], to complex64 [..., n] by the plain conversion, no scaling -- int16 / int8:
    ((float)i, (float)q); uint8 (offset binary): ((float)i - 127.5, (float)q - 127.5); fc32: the float32 pairs (or complex64) as they
    are.  Every value is exact in binary32.  Recc.push_raw_shared_as(a, format) IS Recc.push_raw_shared(convert_samples(a, format)),
    and so for the other three _as calls.  It is the definition for the wideband seam too: Recc.push_wideband_as(a, format) IS
    Recc.push_wideband(convert_samples(a, format)), and Recc.debug_channelize_as likewise.  A dtype that does not match the format
    is a TypeError, never a cast."""
    if format not in SAMPLE_DTYPES:
        raise ValueError("unknown sample format %r" % (format,))
    if not isinstance(a, np.ndarray):
        raise TypeError("convert_samples takes a numpy array, not %s" % type(a).__name__)
    if format == SAMPLES_FC32 and a.dtype == np.complex64:
        return a
    if a.dtype != SAMPLE_DTYPES[format]:
        raise TypeError("sample format %d takes %s samples, not %s" % (format, SAMPLE_DTYPES[format], a.dtype))
    if a.ndim == 0 or (a.shape[-1] != 2 or a.ndim < 2) and a.shape[-1] % 2:
        raise TypeError("samples are [..., n, 2] or [..., 2n], not %r" % (a.shape,))
    pairs = a if a.ndim >= 2 and a.shape[-1] == 2 else a.reshape(a.shape[:-1] + (a.shape[-1] // 2, 2))
    f = pairs.astype(np.float32)
    if format == SAMPLES_CU8:
        f -= np.float32(127.5)
    return np.ascontiguousarray(f).view(np.complex64)[..., 0]


def _typed_block(iq, format, rows, who):
    """A block of `format` for an _as entry point -> (contiguous array or tensor, samples per row).  rows = None: one row, shaped
    [n, 2] or [2n]; else [rows, n, 2] or [rows, 2n].  fc32 blocks may also be complex64 ([n] / [rows, n]).  Anything else is a TypeError."""
    if format not in SAMPLE_DTYPES:
        return iq, None                                   # the library answers -EINVAL: the binding does not second-guess it
    want = SAMPLE_DTYPES[format]
    if isinstance(iq, np.ndarray):
        dt, is_complex = iq.dtype, iq.dtype == np.complex64
    elif hasattr(iq, "data_ptr") and hasattr(iq, "is_cuda"):
        import torch
        if not iq.is_cuda:
            raise TypeError("%s takes a numpy array or a CUDA tensor, not a tensor on %s" % (who, iq.device))
        is_complex = iq.dtype == torch.complex64
        dt = np.dtype(str(iq.dtype).replace("torch.", "")) if not iq.is_complex() else np.dtype(np.complex64)
    else:
        raise TypeError(type(iq))
    if not (dt == want or (format == SAMPLES_FC32 and is_complex)):
        raise TypeError("%s with sample format %d takes %s samples, not %s" % (who, format, want, dt))
    shape = tuple(iq.shape)
    lead = 0 if rows is None else 1
    if rows is not None and (len(shape) < 2 or shape[0] != rows):
        raise TypeError("%s takes %d rows, not shape %r" % (who, rows, shape))
    if is_complex:
        ok, n = len(shape) == lead + 1, shape[-1] if shape else 0
    elif len(shape) == lead + 2 and shape[-1] == 2:
        ok, n = True, shape[-2]
    else:
        ok, n = len(shape) == lead + 1 and shape[-1] % 2 == 0, (shape[-1] // 2 if shape else 0)
    if not ok:
        raise TypeError("%s takes shape %s[n, 2] or %s[2n], not %r" % (who, "[rows, " if lead else "", "[rows, " if lead else "", shape))
    return (np.ascontiguousarray(iq) if isinstance(iq, np.ndarray) else iq.contiguous()), n


class Recc:
    """One handle = `n_channels` independent RECC receivers on one MI355X."""

    def __init__(self, n_channels=1, sps=None, max_samples=0, max_bursts=1024, device=-1, time_kernels=False,
                 stream=None, wideband=None, majority=False, unfused_wideband=False, sync_tolerance=0, slicer="default",
                 sync_torch=True, keep_bursts=False, fixed_timing=False, channel_power=False, stream_power=False, stream_offset=False,
                 seizure_events=False, early_messages=False):
        L = load()
        if stream_offset not in (False, True, "unit"):                     # True: the amplitude-weighted sums; "unit": the unit-amplitude ones
            raise ValueError("stream_offset must be False, True or 'unit'")
        if isinstance(slicer, bool) or slicer not in _SLICER_FLAGS:        # a typo must not run a different numeric spec silently
            raise ValueError("slicer must be one of %r" % sorted(map(str, _SLICER_FLAGS)))
        self.slicer = SLICER_NAMES[L.amps_recc_default_slicer()] if _SLICER_FLAGS[slicer] == 0 else \
            {FLAG_SLICER_ATAN: "atan", FLAG_SLICER_PRODUCT: "product", FLAG_SLICER_SINE: "sine", FLAG_SLICER_EXACT: "exact"}[_SLICER_FLAGS[slicer]]
        self.sync_torch = sync_torch
        if wideband:
            # "decim" absent / 0 = the library default (3/4 of the channels at the narrow banks: the same ratio); the samples per symbol
            # follow the decimation unless they are given
            wideband = dict(wideband)
            # the banks of 10 kHz bins (GRID10_CHANNELS at decim = channels / 4, which has to be stated): two samples per symbol, three
            # taps per branch.  Without a decim they are filled in like any other size below 1024, and the library refuses the result
            if int(wideband["channels"]) in GRID10_CHANNELS and 4 * int(wideband.get("decim") or 0) == int(wideband["channels"]):
                wideband.setdefault("taps_per_branch", 3)
                if sps is None:
                    sps = 2
            if not wideband.get("decim"):
                if int(wideband["channels"]) < 1024:
                    wideband["decim"] = 3 * int(wideband["channels"]) // 4
                else:
                    wideband["decim"] = int(L.amps_recc_default_wideband_decim())
            if sps is None:
                sps = 3 * int(wideband["channels"]) // (2 * int(wideband["decim"]))
        elif sps is None:
            sps = 10
        cfg = Cfg()
        cfg.struct_size = C.sizeof(Cfg)
        cfg.n_channels = n_channels
        cfg.samples_per_symbol = sps
        cfg.max_samples_per_push = max_samples
        cfg.max_bursts = max_bursts
        cfg.device = device
        cfg.flags = ((FLAG_TIME_KERNELS if time_kernels else 0) | (FLAG_MAJORITY if majority else 0)
                     | (FLAG_UNFUSED_WIDEBAND if unfused_wideband else 0)
                     | _SLICER_FLAGS[slicer]
                     | (FLAG_KEEP_BURSTS if keep_bursts else 0) | (FLAG_FIXED_TIMING if fixed_timing else 0)
                     | (FLAG_CHANNEL_POWER if channel_power else 0) | (FLAG_STREAM_POWER if stream_power else 0)
                     | (FLAG_STREAM_OFFSET_UNIT if stream_offset == "unit" else FLAG_STREAM_OFFSET if stream_offset else 0)
                     | (FLAG_SEIZURE_EVENTS if seizure_events else 0) | (FLAG_EARLY_MESSAGES if early_messages else 0))
        cfg.stream = stream
        cfg.sync_tolerance = sync_tolerance
        if wideband:
            cfg.wideband_channels = wideband["channels"]
            cfg.wideband_decim = wideband["decim"]
            cfg.wideband_taps_per_branch = wideband.get("taps_per_branch", 8)
            cfg.wideband_first_channel = wideband.get("first_channel", 0)
            cfg.wideband_groups = wideband.get("groups", 0)
            cfg.wideband_group = wideband.get("group", 0)
        self.n_channels, self.sps, self.max_bursts, self.max_samples = n_channels, sps, max_bursts, max_samples
        self.decim = int(wideband["decim"]) if wideband else None
        self.resample = None                                   # (interp, decim) of the wideband seam's resampler, where one is set
        self._origin = 0
        self._h = C.c_void_p()
        rc = L.amps_recc_create(C.byref(self._h), C.byref(cfg))
        if rc != 0:
            self._h = None
            raise AmpsError(rc, "amps_recc_create")
        if wideband and wideband.get("resample"):              # (rate_hz, interp, decim): blocks arrive at rate_hz
            try:
                self.set_wideband_resample(*wideband["resample"])
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.amps_recc_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        _call("amps_recc_reset", self._h)
        self._origin = 0

    def _tap(self, name, rows, cap, *args):
        """a test tap: entry point `name`(handle, *args, out, cap, &nout) fills complex64 [rows][cap] ([cap] with rows = None) -> the
        nout it delivered of every row"""
        out = np.zeros(cap if rows is None else (rows, cap), np.complex64)
        nout = C.c_size_t(0)
        _call(name, self._h, *args, _hostptr(out), cap, C.byref(nout))
        return out[..., :nout.value].copy()

    def _records(self, name, cap, *tail, symbols=None, shared=False, copy=True):
        """a drain: entry point `name`(handle, out, [symbols,] cap, &nout, *tail) -> the nout records.  shared: into the handle's
        own buffer, which copy=False hands out as a view; otherwise into a fresh one"""
        if shared:
            out = getattr(self, "_drain_buf", None)
            if out is None or out.shape[0] < cap:
                out = self._drain_buf = np.empty(cap, BURST_DTYPE)
        else:
            out = np.empty(cap, BURST_DTYPE)
        nout = C.c_size_t(0)
        _call(name, self._h, _hostptr(out), *(() if symbols is None else (_hostptr(symbols),)), cap, C.byref(nout), *tail)
        return out[:nout.value].copy() if copy else out[:nout.value]

    # ---- seam (i): recc::work ----
    def push_symbols(self, syms, n=None):
        """syms: uint8 [C][ld] (numpy or torch cuda). One work() call per channel with noutput_items=n.
        Returns (bursts uint8 [k][3374], channels uint32 [k])."""
        if isinstance(syms, np.ndarray):
            syms = np.ascontiguousarray(syms, np.uint8)
        syms2 = syms.reshape(self.n_channels, -1)
        ld = syms2.shape[1]
        n = ld if n is None else n
        ptr, mem, keep = _as_ptr(syms2, self.sync_torch)
        out = np.zeros((self.max_bursts, CAPTURE), np.uint8)
        ch = np.zeros(self.max_bursts, np.uint32)
        nout = C.c_size_t(0)
        _call("amps_recc_push_symbols", self._h, ptr, ld, n, mem, _hostptr(out), _hostptr(ch), self.max_bursts, C.byref(nout))
        return out[:nout.value].copy(), ch[:nout.value].copy()

    def decode_bursts(self, bursts, channels=None):
        if isinstance(bursts, np.ndarray):
            bursts = np.ascontiguousarray(bursts, np.uint8).reshape(-1, CAPTURE)
        nb = bursts.shape[0]
        out = np.zeros(nb, BURST_DTYPE)
        if nb == 0:
            return out
        ptr, mem, keep = _as_ptr(bursts, self.sync_torch)
        chp = None
        if channels is not None:
            channels = np.ascontiguousarray(channels, np.uint32)
            chp = _hostptr(channels)
        _call("amps_recc_decode_bursts", self._h, ptr, nb, mem, chp, _hostptr(out))
        return out

    # ---- seam (ii): fused IQ ----
    def push_iq(self, iq, nsamp=None):
        """iq: complex64 [C][ld] numpy array, or torch cuda tensor (complex64 [C][ld] or float32 [C][ld][2])."""
        iq, ld = _fc32_rows(iq, self.n_channels)
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        _call("amps_recc_push_iq", self._h, ptr, ld, ld if nsamp is None else nsamp, mem)

    def set_xlate(self, rate_hz=400e3, center_hz=160e3, decim=2, gain=0.0, cutoff_hz=0.0, width_hz=0.0):
        """Put the reference flow graph's channel filter (freq_xlating_fir_filter_ccc, grc/recctest.grc:889-937)
        in front of the IQ seam; zeros select the flow graph's gain / cutoff / transition width."""
        x = XlateCfg(C.sizeof(XlateCfg), decim, rate_hz, center_hz, gain, cutoff_hz, width_hz)
        _call("amps_recc_set_xlate", self._h, C.byref(x))

    def push_raw(self, iq, nsamp=None):
        """like push_iq, at the translate stage's input rate (e.g. the 400 ksps .raw captures of recctest.grc)."""
        iq, ld = _fc32_rows(iq, self.n_channels)
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        _call("amps_recc_push_raw", self._h, ptr, ld, ld if nsamp is None else nsamp, mem)

    def debug_xlate(self, iq):
        """Translate stage only (test tap): complex64 [C][n] -> complex64 [C][nout]."""
        iq, n = _fc32_rows(iq, self.n_channels)
        ptr, mem, keep = _as_ptr(iq)
        return self._tap("amps_recc_debug_xlate", self.n_channels, n + 8, ptr, n, n, mem)

    # ---- translate seam, shared form: many channels of one narrowband stream
    def set_xlate_shared(self, rate_hz, centers_hz, decim, gain=0.0, cutoff_hz=0.0, width_hz=0.0):
        """Channel c of the handle = the channel at centers_hz[c] (relative to the stream's centre) of ONE shared stream at rate_hz:
        the flow graph's channel filter per centre, all of them in one launch, in front of the IQ seam (amps_recc_set_xlate_shared).
        len(centers_hz) must be n_channels; zeros select the flow graph's gain / cutoff / transition width; decim 0 removes the stage.
        decim is 1, 2, 4 or 8 (filters of up to 1280 taps) or 5, 6, 10, 12, 16 or 20 (up to 2400: the default filter to 3.2 Msps), and
        rate_hz / decim must be the handle's sps x 20 kHz: subband_plan(rate_hz) lists the (decim, sps) pairs a rate admits."""
        cen = np.ascontiguousarray(centers_hz, np.float64).reshape(-1)
        x = XlateSharedCfg(C.sizeof(XlateSharedCfg), int(decim), cen.size, 0, rate_hz, gain, cutoff_hz, width_hz,
                           cen.ctypes.data_as(C.POINTER(C.c_double)))
        _call("amps_recc_set_xlate_shared", self._h, C.byref(x))

    def retune_xlate(self, centers_hz):
        """Replace the centres of the configured translate form in mid-stream (amps_recc_retune_xlate): n_channels centres for the
        shared and the resampled form, one for the per-row form.  Takes effect with the next push; from then on the stage delivers,
        bit for bit, what a handle configured with these centres from the start would.  Nothing is reset and the host does not wait."""
        cen = np.ascontiguousarray(centers_hz, np.float64).reshape(-1)
        _call("amps_recc_retune_xlate", self._h, cen.ctypes.data_as(C.POINTER(C.c_double)), cen.size)

    def set_wideband_shift(self, shift_hz):
        """Correct a tuner's frequency error inside the filter bank (amps_recc_set_wideband_shift; the banks below 1024 branches):
        shift_hz is the frequency in the delivered stream of what shall land on bin 0's centre, so a radio that delivers everything
        e hertz too high gets +e.  Takes effect with the next push; from then on the bank delivers, bit for bit, what a handle with
        this shift from the start would.  Nothing is reset and the host does not wait; 0 runs the unmixed kernels again."""
        _call("amps_recc_set_wideband_shift", self._h, float(shift_hz))

    @property
    def wideband_shift(self):
        """The shift in force in hertz, as quantised to the mixer's step (amps_recc_wideband_shift)."""
        hz = C.c_double(0.0)
        _call("amps_recc_wideband_shift", self._h, C.byref(hz))
        return hz.value

    def set_wideband_resample(self, rate_hz, interp, decim, cutoff_hz=0.0, width_hz=0.0):
        """The wideband seam for a rate that is no bank's: blocks arrive at rate_hz and are resampled by interp / decim to the bank's
        rate on their way into the filter bank (amps_recc_set_wideband_resample; 8 Msps x 5/4 into the 1000 bank, 12.5 Msps x 2/1
        into the 2500 bank, ...).  interp and decim are 1 ... 8 and coprime, 1/2 <= interp / decim <= 4; wideband_resample_plan(rate_hz)
        lists what a rate admits.  Every push_wideband* and debug_channelize* then takes blocks at rate_hz; decim 0 removes the stage.
        Before the first push, or after reset()."""
        x = WidebandResampleCfg(C.sizeof(WidebandResampleCfg), int(interp), int(decim), 0, float(rate_hz), float(cutoff_hz), float(width_hz))
        _call("amps_recc_set_wideband_resample", self._h, C.byref(x))
        self.resample = (int(interp), int(decim)) if int(decim) else None

    def debug_wideband_resample(self, iq, format=SAMPLES_FC32):
        """The resampler only (test tap), continuing its stream: a block in `format` at the delivered rate -> complex64 [nout] at the
        bank's rate."""
        if format == SAMPLES_FC32 and isinstance(iq, np.ndarray) and iq.dtype == np.complex64:
            iq, n = _fc32_row(iq)                              # of any shape, flattened
        else:
            iq, n = _typed_block(iq, format, None, "debug_wideband_resample")
        n = n or 0
        ptr, mem, keep = _as_ptr(iq)
        interp, decim = self.resample or (1, 1)
        return self._tap("amps_recc_debug_wideband_resample", None, n * interp // decim + 2, ptr, n, format, mem)

    def _bank_samples(self, n):
        """samples at the bank's rate that n delivered samples come to at the most"""
        return n if not self.resample else n * self.resample[0] // self.resample[1] + 1

    def set_xlate_resampled(self, rate_hz, centers_hz, interp, decim, gain=0.0, cutoff_hz=0.0, width_hz=0.0):
        """set_xlate_shared for the rates no integer decimation serves: the shared stream is resampled by interp / decim (2.048 Msps
        x 5/64, 2.5 Msps x 2/25, ...) to the handle's sps x 20 kHz by a polyphase resampler behind the per-channel mix
        (amps_recc_set_xlate_resampled).  interp is 2 ... 5, decim up to 64 and coprime to it; resample_plan(rate_hz) lists the
        (interp, decim, sps) a rate admits.  push_raw_shared[_as] and debug_xlate_shared[_as] then run this stage; decim 0 removes it."""
        cen = np.ascontiguousarray(centers_hz, np.float64).reshape(-1)
        x = XlateResampleCfg(C.sizeof(XlateResampleCfg), int(interp), int(decim), cen.size, 0, rate_hz, gain, cutoff_hz, width_hz,
                             cen.ctypes.data_as(C.POINTER(C.c_double)))
        _call("amps_recc_set_xlate_resampled", self._h, C.byref(x))

    @staticmethod
    def _one_row(iq):
        """_fc32_row for the shared stream, which refuses a tensor that is not one row"""
        if not isinstance(iq, np.ndarray):
            if iq.dim() != 1 and not (iq.dim() == 2 and iq.shape[-1] == 2 and not iq.is_complex()):
                raise TypeError("the shared stream is one row: a 1-D complex64 tensor, not shape %r" % (tuple(iq.shape),))
            iq = iq.contiguous()
        return _fc32_row(iq)

    def push_raw_shared(self, iq):
        """one block of the shared stream: a 1-D complex64 numpy array (staged) or torch device tensor (read in place)"""
        iq, n = self._one_row(iq)
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        _call("amps_recc_push_raw_shared", self._h, ptr, n, mem)

    def debug_xlate_shared(self, iq):
        """Shared translate stage only (test tap): complex64 [n] -> complex64 [C][nout]."""
        iq, n = self._one_row(iq)
        ptr, mem, keep = _as_ptr(iq)
        return self._tap("amps_recc_debug_xlate_shared", self.n_channels, n + 8, ptr, n, mem)

    # ---- translate seams on an SDR's integer samples (sc16, sc8, cu8), read in place: include/amps_recc.h, AMPS_RECC_SAMPLES_*
    def push_raw_shared_as(self, iq, format):
        """push_raw_shared on a block in `format` (SAMPLES_*): a numpy array of the format's dtype shaped [n, 2] or [2n] (staged as it
        is) or a torch device tensor of that dtype (read in place).  By definition push_raw_shared(convert_samples(iq, format)); a
        dtype that does not match the format is a TypeError, never a cast."""
        iq, n = _typed_block(iq, format, None, "push_raw_shared_as")
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        _call("amps_recc_push_raw_shared_as", self._h, ptr, n or 0, format, mem)

    def debug_xlate_shared_as(self, iq, format):
        """Shared translate stage only (test tap) on a block in `format`: [n, 2] or [2n] -> complex64 [C][nout]."""
        iq, n = _typed_block(iq, format, None, "debug_xlate_shared_as")
        n = n or 0
        ptr, mem, keep = _as_ptr(iq)
        return self._tap("amps_recc_debug_xlate_shared_as", self.n_channels, n + 8, ptr, n, format, mem)

    def push_raw_as(self, iq, format, nsamp=None):
        """push_raw on rows in `format`: [C, n, 2] or [C, 2n] of the format's dtype, numpy or torch device tensor; the first nsamp
        samples of each row (default: all n, the row pitch)."""
        iq, ld = _typed_block(iq, format, self.n_channels, "push_raw_as")
        ld = ld or 0
        nsamp = ld if nsamp is None else nsamp
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        _call("amps_recc_push_raw_as", self._h, ptr, ld, nsamp, format, mem)

    def debug_xlate_as(self, iq, format, nsamp=None):
        """Translate stage only (test tap) on rows in `format`: [C, n, 2] or [C, 2n] -> complex64 [C][nout]."""
        iq, ld = _typed_block(iq, format, self.n_channels, "debug_xlate_as")
        ld = ld or 0
        nsamp = ld if nsamp is None else nsamp
        ptr, mem, keep = _as_ptr(iq)
        return self._tap("amps_recc_debug_xlate_as", self.n_channels, nsamp + 8, ptr, ld, nsamp, format, mem)

    def push_wideband(self, iq):
        iq, n = _fc32_row(iq)
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        _call("amps_recc_push_wideband", self._h, ptr, n, mem)

    def push_wideband_short(self, iq):
        """The wideband block as interleaved 16-bit I/Q (amps_recc_push_wideband_short): a numpy int16 array of shape [n, 2] or [2n], or
        a torch int16 CUDA tensor of the same shapes (read in place, like push_wideband's device blocks).  Nothing else is taken: a
        float array is a TypeError, not a silent cast."""
        iq, n = _typed_block(iq, SAMPLES_SC16, None, "push_wideband_short")
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        _call("amps_recc_push_wideband_short", self._h, ptr, n, mem)

    # ---- wideband seam on an SDR's integer samples (sc16, sc8, cu8), read in place: include/amps_recc.h, amps_recc_push_wideband_as
    def push_wideband_as(self, iq, format):
        """push_wideband on a block in `format` (SAMPLES_*): a numpy array of the format's dtype shaped [n, 2] or [2n] (staged as it
        is, 2 bytes per sample for sc8 and cu8) or a torch device tensor of that dtype (read in place).  By definition
        push_wideband(convert_samples(iq, format)); a dtype that does not match the format is a TypeError, never a cast."""
        iq, n = _typed_block(iq, format, None, "push_wideband_as")
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        _call("amps_recc_push_wideband_as", self._h, ptr, n or 0, format, mem)

    def debug_channelize_as(self, iq, format):
        """Channelizer only (test tap) on a block in `format`: [n, 2] or [2n] -> complex64 [C][nframes]."""
        iq, n = _typed_block(iq, format, None, "debug_channelize_as")
        n = n or 0
        ptr, mem, keep = _as_ptr(iq)
        cap = self._bank_samples(n) // min(512, self.decim or 512) + 6          # as debug_channelize
        return self._tap("amps_recc_debug_channelize_as", self.n_channels, cap, ptr, n, format, mem)

    # ---- one band over the GPUs of a node: RCCL inside the C ABI (include/amps_recc.h, amps_recc_push_wideband_bcast)
    @staticmethod
    def rccl_unique_id():
        """128 bytes from ncclGetUniqueId: one rank makes them, the application carries them to the others"""
        buf = (C.c_uint8 * 128)()
        _call("amps_recc_rccl_unique_id", buf)
        return bytes(buf)

    def rccl_init(self, uid, nranks, rank):
        """collective: returns when all nranks handles (one per GPU / process) have joined"""
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _call("amps_recc_rccl_init", self._h, buf, int(nranks), int(rank))

    def push_wideband_dist(self, iq, nsamp=None, root=0, mode="broadcast"):
        """every rank in step; the root passes its block (a CUDA tensor, used in place, or a numpy array, staged), the others None.
        mode: "broadcast" (flat ncclBroadcast) or "scatter_allgather".  Returns the number of samples pushed: the ROOT's, on every rank.
        The root passing None ends the stream: every rank's call raises AmpsError with code -errno.ENODATA, nothing is pushed."""
        ptr, mem, n = None, MEM_DEVICE, 0
        if iq is not None:
            iq, _ = _fc32_row(iq)
            have = int(iq.numel()) if hasattr(iq, "numel") else int(iq.size)      # complex samples
            n = have if nsamp is None else int(nsamp)
            if n > have:                                   # the C side would read past the end of the buffer
                raise ValueError("nsamp = %d exceeds the %d complex samples of the block" % (n, have))
            ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        pushed = C.c_size_t(0)
        _call("amps_recc_push_wideband_dist", self._h, ptr, n, mem, int(root), DIST_MODES[mode], C.byref(pushed))
        return int(pushed.value)

    def push_wideband_bcast(self, iq, nsamp=None, root=0):
        """push_wideband_dist(mode="broadcast"): the round-4 entry point"""
        return self.push_wideband_dist(iq, nsamp, root, "broadcast")

    def rccl_abort(self):
        """this rank leaves: its communicator is aborted, the peers' bounded waits end with -ETIMEDOUT"""
        _call("amps_recc_rccl_abort", self._h)

    def rccl_set_timeout(self, milliseconds):
        _call("amps_recc_rccl_set_timeout", self._h, int(milliseconds))

    def rccl_info(self):
        """the communicator as RCCL reports it + the device it runs on + the timed data collectives, as a dict"""
        info = RcclInfo()
        info.struct_size = C.sizeof(RcclInfo)
        _call("amps_recc_rccl_info", self._h, C.byref(info))
        d = {k: getattr(info, k) for k, _ in RcclInfo._fields_ if k not in ("struct_size", "_pad", "device_uuid", "library")}
        d["device_uuid"] = bytes(info.device_uuid).hex()
        d["library"] = info.library.decode(errors="replace")
        d["last_mode"] = {0: "broadcast", 1: "scatter_allgather"}.get(info.last_mode)
        d["collective_gbps"] = (info.collective_bytes / (info.collective_ms * 1e-3) / 1e9) if info.collective_ms > 0 else None
        return d

    def drain_gather(self, root=0, cap=None):
        """every rank in step: each drains its own list, the root returns the records of ALL ranks sorted by (channel, position)
        (what one whole-band handle would have drained), the others an empty array"""
        return self._records("amps_recc_drain_gather", cap or self.max_bursts, int(root))

    def refchain_symbols(self, iq):
        """The flow graph's own sub-chain (quadrature_demod_cf -> clock_recovery_mm_ff -> binary_slicer_fb) on the device:
        complex64 [C][n] at 200 ksps -> list of uint8 symbol arrays, one per channel (continues across calls)."""
        iq, n = _fc32_rows(iq, self.n_channels)
        ptr, mem, keep = _as_ptr(iq, self.sync_torch)
        cap = n // 9 + 16
        out = np.zeros((self.n_channels, cap), np.uint8)
        ns = np.zeros(self.n_channels, np.uint32)
        _call("amps_recc_refchain_symbols", self._h, ptr, n, n, mem, _hostptr(out), cap, _hostptr(ns))
        return [out[c, :ns[c]].copy() for c in range(self.n_channels)]

    def refchain_tables(self):
        a, m = np.zeros(258, np.float32), np.zeros((129, 8), np.float32)
        _call("amps_recc_refchain_tables", self._h, _hostptr(a), _hostptr(m))
        return a, m

    def wait_torch(self, stream=None):
        """Order later pushes behind everything enqueued so far on a torch CUDA stream (default: the current one), without
        blocking the host: an event is recorded on that stream and the handle's stream waits for it."""
        import torch
        ev = torch.cuda.Event()
        ev.record(stream or torch.cuda.current_stream())
        _call("amps_recc_wait_event", self._h, C.c_void_p(ev.cuda_event))
        self._keep_ev = ev

    def record_torch_event(self):
        """The converse: a torch event recorded behind everything this handle has enqueued so far; a torch stream that
        waits for it (stream.wait_event) may then overwrite a buffer the handle's kernels read."""
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())          # creates the underlying hipEvent_t
        _call("amps_recc_record_event", self._h, C.c_void_p(ev.cuda_event))
        return ev

    def bch_encode(self, msg_bits):
        """uint8 [n][k] message bits -> uint8 [n][k+12] code words (k = 28: FOCC/FVC, k = 36: RECC)."""
        m = np.ascontiguousarray(msg_bits, np.uint8)
        n, k = m.shape
        out = np.zeros((n, k + 12), np.uint8)
        _call("amps_bch_encode_words", self._h, _hostptr(m), n, k, MEM_HOST, _hostptr(out))
        return out

    def bch_decode(self, codewords):
        """uint8 [n][k+12] -> (msg uint8 [n][k], valid uint8 [n], nerrors uint8 [n])."""
        c = np.ascontiguousarray(codewords, np.uint8)
        n, nb = c.shape
        k = nb - 12
        msg, valid, nerr = np.zeros((n, k), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        _call("amps_bch_decode_words", self._h, _hostptr(c), n, k, MEM_HOST, _hostptr(msg), _hostptr(valid), _hostptr(nerr))
        return msg, valid, nerr

    def debug_channelize(self, iq):
        """Channelizer only (test tap): wideband complex64 [n] -> complex64 [C][nframes]."""
        iq, n = _fc32_row(iq)
        ptr, mem, keep = _as_ptr(iq)
        cap = self._bank_samples(n) // min(512, self.decim or 512) + 6          # the frames of the block, and up to four whose samples waited in the carry
        return self._tap("amps_recc_debug_channelize", self.n_channels, cap, ptr, n, mem)

    def drain(self, cap=None, copy=True):
        """Synchronise and return the decoded bursts since the last drain, sorted by (channel, position).
        copy=False returns a view of a buffer owned by this handle, valid until the next drain()."""
        return self._records("amps_recc_drain", cap or self.max_bursts, shared=True, copy=copy)

    def drain_bursts(self, cap=None):
        """drain() plus the 3374 captured symbol bytes of every record (handle created with keep_bursts=True)"""
        cap = cap or self.max_bursts
        sym = np.zeros((cap, CAPTURE), np.uint8)
        recs = self._records("amps_recc_drain_bursts", cap, symbols=sym)
        return recs, sym[:len(recs)].copy()

    def drain_seizures(self, cap=None):
        """The seizure events held (handle created with seizure_events=True), oldest first, as a SEIZURE_DTYPE array ordered by
        (found_at, channel): one per seizure, available after the push in which its trigger was accepted, long before its record
        (amps_recc_drain_seizures).  At most `cap` (default max_bursts) are taken; the rest stay for the next call.  If events were
        dropped because the list was full, the AmpsError (-errno.ENOSPC) carries what was delivered as its `seizures` attribute."""
        cap = self.max_bursts if cap is None else int(cap)
        out = np.zeros(cap, SEIZURE_DTYPE)
        nout, nleft = C.c_size_t(0), C.c_size_t(0)
        try:
            _call("amps_recc_drain_seizures", self._h, _hostptr(out) if cap else None, cap, C.byref(nout), C.byref(nleft))
        except AmpsError as e:
            e.seizures = out[:nout.value].copy()
            raise
        return out[:nout.value].copy()

    def drain_early(self, cap=None):
        """The early messages held (handle created with early_messages=True), oldest first, as an EARLY_DTYPE array ordered by
        (found_at, channel): per seizure whose word A announced fewer than seven words, the record of those words (`rec`, a
        BURST_DTYPE: what the later record will carry for them, bit for bit), available after the push in which the last repeat of the
        last of them arrived (amps_recc_drain_early).  At most `cap` (default max_bursts) are taken; the rest stay for the next call.
        If events were dropped because the list was full, the AmpsError (-errno.ENOSPC) carries what was delivered as its `early`
        attribute."""
        cap = self.max_bursts if cap is None else int(cap)
        out = np.zeros(cap, EARLY_DTYPE)
        nout, nleft = C.c_size_t(0), C.c_size_t(0)
        try:
            _call("amps_recc_drain_early", self._h, _hostptr(out) if cap else None, cap, C.byref(nout), C.byref(nleft))
        except AmpsError as e:
            e.early = out[:nout.value].copy()
            raise
        return out[:nout.value].copy()

    def set_origin(self, first_sample):
        """absolute index of the first sample pushed after create / reset (multiple of 64)"""
        _call("amps_recc_set_origin", self._h, first_sample)
        self._origin = int(first_sample)

    def drain_begin(self):
        """Close the current record list without waiting; pushes issued after this append to a second list."""
        _call("amps_recc_drain_begin", self._h)

    def drain_end(self, cap=None, copy=True):
        """Wait for the work enqueued before drain_begin() only, and return its records (sorted)."""
        return self._records("amps_recc_drain_end", cap or self.max_bursts, shared=True, copy=copy)

    def debug_demod(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        n = iq.size
        d, s, g = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
        _call("amps_recc_debug_demod", self._h, _hostptr(iq), n, MEM_HOST, _hostptr(d), _hostptr(s), _hostptr(g))
        p = (n // 64) * 64
        return d[:p], s[:p], g[:p]

    def debug_slicer_bits(self, first, n):
        """Test tap of the slicer bit ring: (bits uint8 [rows][n], produced) -- the bits of absolute samples [first, first + n) of
        every ring row once the pushes so far have finished, and one past the last sample produced (amps_recc_debug_slicer_bits)."""
        rows, produced = C.c_uint32(0), C.c_uint64(0)
        _call("amps_recc_debug_slicer_bits", self._h, 0, 0, None, 0, C.byref(rows), C.byref(produced))
        out = np.zeros((rows.value, n), np.uint8)
        if n:
            _call("amps_recc_debug_slicer_bits", self._h, first, n, _hostptr(out), n, C.byref(rows), C.byref(produced))
        return out, produced.value

    # ---- received power: of the wideband seam (handles created with channel_power=True: one snapshot every 256 frames) and of the IQ
    # and translate seams (stream_power=True: the mean of every block of 256 channel-rate samples)
    @property
    def power_ring_snaps(self):
        """snapshots / blocks the handle keeps per row (the slicer-bit ring's span / 256); 0 without channel_power or stream_power"""
        return int(load().amps_recc_power_ring_snaps(self._h))

    def channel_power(self, first=None, n=None):
        """(float32 [rows][n], first): P[row][first + i], linear and unscaled, once the pushes so far have finished
        (amps_recc_channel_power).  Wideband seam (channel_power): |filter-bank output|^2 of the frame at channel-rate sample
        256 (first + i).  IQ and translate seams (stream_power): the mean of |y|^2 over the channel-rate samples [256 (first + i),
        256 (first + i + 1)), which exists once the whole block has been sliced.  Default: everything currently held -- on either seam
        [max(ceil(origin / 256), produced - ring), produced), `produced` as the library reports it; `first` alone: from there to the
        newest."""
        return self._ring_rows("amps_recc_channel_power", self.power_ring_snaps, np.float32, first, n)

    def _ring_rows(self, name, ring_slots, dtype, first, n):
        """channel_power / channel_autocorr: ask what is produced, default to the held window, allocate, fetch"""
        rows, prod = C.c_uint32(0), C.c_uint64(0)
        _call(name, self._h, 0, 0, None, 0, C.byref(rows), C.byref(prod))
        if first is None:
            first = max(-(-self._origin // POWER_STRIDE), prod.value - ring_slots)      # the held window's first entry
        if n is None:
            n = max(0, prod.value - first)
        out = np.zeros((rows.value, n), dtype)
        if n:
            _call(name, self._h, first, n, _hostptr(out), n, None, None)
        return out, int(first)

    def _ring_bursts(self, name, records, dtype):
        """burst_power / burst_autocorr / burst_offset: records in, one value and one count per record out"""
        recs = np.ascontiguousarray(records, BURST_DTYPE).reshape(-1)
        val, cnt = np.zeros(recs.size, dtype), np.zeros(recs.size, np.uint32)
        _call(name, self._h, _hostptr(recs), recs.size, _hostptr(val), _hostptr(cnt))
        return val, cnt

    def burst_power(self, records):
        """(mean float32 [n], count uint32 [n]) for records as drain() returns them: the mean power snapshot (wideband seam) or power
        block (IQ and translate seams) of each record's channel over its capture and the number averaged, (0.0, 0) where the ring no
        longer (or not yet) holds them (amps_recc_burst_power)"""
        return self._ring_bursts("amps_recc_burst_power", records, np.float32)

    # ---- carrier offset of the IQ and translate seams (handles created with stream_offset=True, or "unit" for the unit-amplitude
    # statistic, which is the one to use behind a channel filter): the lag-one autocorrelation sum of
    # every block of 256 channel-rate samples, and its sum and argument over a record's capture
    @property
    def autocorr_ring_blocks(self):
        """blocks the handle keeps per row: the slicer-bit ring's span R / 256, R the smallest power of two >= max_samples + sps * 3586
        + 1024 (include/amps_recc.h: amps_recc_debug_slicer_bits)"""
        need, span = self.max_samples + self.sps * 3586 + 1024, 1
        while span < need:
            span <<= 1
        return span // POWER_STRIDE

    def channel_autocorr(self, first=None, n=None):
        """(complex64 [rows][n], first): A[row][first + i] = 2^-8 sum of y[s] conj(y[s - 1]) (stream_offset="unit": of those products
        brought to unit amplitude, U) over the channel-rate samples
        [256 (first + i), 256 (first + i + 1)), once the pushes so far have finished (amps_recc_channel_autocorr).  Default: everything
        currently held, as channel_power on a stream_power handle"""
        return self._ring_rows("amps_recc_channel_autocorr", self.autocorr_ring_blocks, np.complex64, first, n)

    def burst_autocorr(self, records):
        """(sum complex64 [n], count uint32 [n]) for records as drain() returns them: the sum of A over the blocks wholly inside each
        record's capture and their number, (0, 0) where the ring no longer (or not yet) holds them (amps_recc_burst_autocorr)"""
        return self._ring_bursts("amps_recc_burst_autocorr", records, np.complex64)

    def burst_offset(self, records):
        """(offset in Hz float32 [n], count uint32 [n]): the argument of burst_autocorr's sums times fs / 2 pi, fs = 20000 * sps; 0.0
        where nothing is held (amps_recc_burst_offset).  Positive: the mobile is above the channel centre"""
        return self._ring_bursts("amps_recc_burst_offset", records, np.float32)

    def set_timing(self, mode):
        """mode: "off" | "all" | "dominant" (only the streaming kernel of the seam in use is bracketed by HIP events) |
        "sampled" (the dominant kernel of every eighth push)"""
        _call("amps_recc_set_timing", self._h, {"off": 0, "all": 1, "dominant": 2, "sampled": 3}[mode])

    def timing(self, reset=False):
        t = Timing()
        _call("amps_recc_get_timing", self._h, C.byref(t), int(reset))
        return {k: getattr(t, k) for k, _ in Timing._fields_ if k not in ("struct_size", "_pad")}


def reply_words(rec):
    rec = np.ascontiguousarray(rec)
    r = Reply()
    _call("amps_recc_reply_words", _hostptr(rec), C.byref(r))
    return r


def reverse_channel_hz(n):
    """Centre frequency of AMPS reverse (mobile transmit) channel n: 825.000 MHz + 30 kHz n for 1 <= n <= 799, and
    825.000 MHz + 30 kHz (n - 1023) for the extended channels 991 <= n <= 1023."""
    n = int(n)
    if 1 <= n <= 799:
        return 825.0e6 + 30e3 * n
    if 991 <= n <= 1023:
        return 825.0e6 + 30e3 * (n - 1023)
    raise ValueError("no AMPS channel %d (1..799, 991..1023)" % n)


CONTROL_CHANNELS = {"A": range(313, 334), "B": range(334, 355), "AB": range(313, 355)}


def subband_plan(rate_hz, width_hz=0.0):
    """Which decimation for a stream at rate_hz?  The (decim, sps, ntaps) triples Recc.set_xlate_shared accepts for that rate on a
    handle of `sps` samples per symbol, ascending by decim; ntaps is the channel filter's length at transition width width_hz (0 = the
    flow graph's 4.5 kHz).  Empty for a rate no decimation serves (2.048 Msps, or 4 Msps under the default width).  Needs no GPU
    (amps_recc_xlate_shared_plan)."""
    return _plan("amps_recc_xlate_shared_plan", XlatePlan, rate_hz, width_hz)


def wideband_plan(rate_hz):
    """Which filter bank for a wideband stream at rate_hz?  The (channels, decim, sps, taps) Recc(wideband={"channels": .., "decim": ..})
    accepts for that rate, the default decimation first: two for 30.72, 15.36, 7.68 and 3.84 Msps, none for any other rate.  Needs no
    GPU (amps_recc_wideband_plan)."""
    return _plan("amps_recc_wideband_plan", WidebandPlan, rate_hz)


def wideband_grid_plan(rate_hz):
    """wideband_plan for every bank the seam has: (channels, decim, sps, taps, bin_hz, channel_stride, max_channels) per entry.  The
    entries of wideband_plan with (30000, 1, channels) behind them, and for 25, 20, 10 and 5 Msps the bank of rate / 10 kHz branches:
    10e6 -> [(1000, 250, 2, 3000, 10000, 3, 333)], for Recc(wideband={"channels": 1000, "decim": 250}), a channel on every third
    bin.  Needs no GPU (amps_recc_wideband_grid_plan)."""
    return _plan("amps_recc_wideband_grid_plan", WidebandGridPlan, rate_hz)


def wideband_resample_plan(rate_hz):
    """Which ratio into which bank for a wideband stream at a rate wideband_grid_plan has nothing for?  The (interp, decim, channels,
    bank_decim, sps, ntaps_per_phase, bin_hz, channel_stride, usable_hz) Recc(wideband={"channels": .., "decim": .., "resample":
    (rate_hz, interp, decim)}) accepts: 8e6 -> (5, 2, 2000, 500, ...), (5, 4, 1000, 250, ...), (5, 8, 500, 125, ...).  Needs no GPU
    (amps_recc_wideband_resample_plan)."""
    return _plan("amps_recc_wideband_resample_plan", WidebandResamplePlan, rate_hz)


def resample_plan(rate_hz, width_hz=0.0):
    """Which ratio for a stream at rate_hz that subband_plan has no decimation for?  The (interp, decim, sps, ntaps_per_phase)
    Recc.set_xlate_resampled accepts for that rate, ascending by (interp, decim).  Needs no GPU (amps_recc_xlate_resample_plan)."""
    return _plan("amps_recc_xlate_resample_plan", ResamplePlan, rate_hz, width_hz)


def control_channel_centers(system, tuned_hz):
    """The reverse control channels of system "A" (313-333), "B" (334-354) or "AB" (313-354) as centres relative to a receiver
    tuned to tuned_hz: what Recc.set_xlate_shared takes."""
    if system not in CONTROL_CHANNELS:
        raise ValueError("system must be one of %r" % sorted(CONTROL_CHANNELS))
    return [reverse_channel_hz(n) - float(tuned_hz) for n in CONTROL_CHANNELS[system]]
