"""ctypes binding of libp1hip.so (declarations: include/p1hip.h).

Fails loudly: a missing library, a missing symbol or a non-zero return code
raises P1HipError.  Nothing here computes a hash on the CPU.

A process that also uses torch on the GPU must import torch BEFORE the
library is loaded: the torch wheel ships its own HIP runtime, and
libp1hip.so has to bind to that copy; the other order leaves two HIP
runtimes in the process and the second to initialise sees no device.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

U64 = ctypes.c_uint64


class P1HipError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__(f"p1hip rc={rc}: {msg}")
        self.rc = rc


class Stats(ctypes.Structure):
    _fields_ = [
        ("scans", U64),
        ("fast_launches", U64),
        ("fast_nonces", U64),
        ("fast_alg_ops", U64),
        ("generic_launches", U64),
        ("generic_nonces", U64),
        ("scan_wall_ms", ctypes.c_double),
        ("scan_launches", U64),
        ("scan_nonces", U64),
        ("scan_alg_ops", U64),
        ("scan_kernel_ms", ctypes.c_double),
        ("small_scans", U64),
        ("table_replans", U64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DeviceStats(ctypes.Structure):
    _fields_ = [
        ("ordinal", ctypes.c_int32),
        ("active", ctypes.c_int32),
        ("shard_first", U64),
        ("shard_last", U64),
        ("scans", U64),
        ("scan_launches", U64),
        ("scan_nonces", U64),
        ("scan_alg_ops", U64),
        ("scan_kernel_ms", ctypes.c_double),
        ("phase1_ms", ctypes.c_double),
        ("gather_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Request(ctypes.Structure):
    _fields_ = [("msg", ctypes.c_char_p), ("msg_len", ctypes.c_size_t), ("lower", U64), ("upper", U64)]


class Result(ctypes.Structure):
    _fields_ = [("hash", U64), ("nonce", U64)]


class BatchStats(ctypes.Structure):
    _fields_ = [
        ("calls", U64),
        ("requests", U64),
        ("coalesced", U64),
        ("individual", U64),
        ("empty", U64),
        ("launches", U64),
        ("tiles", U64),
        ("nonces", U64),
        ("wall_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class WideStats(ctypes.Structure):
    _fields_ = [
        ("calls", U64),
        ("requests", U64),
        ("empty", U64),
        ("small", U64),
        ("wide", U64),
        ("individual", U64),
        ("scan_launches", U64),
        ("scan_segments", U64),
        ("generic_launches", U64),
        ("generic_segments", U64),
        ("tiles", U64),
        ("nonces", U64),
        ("wall_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AsyncStats(ctypes.Structure):
    _fields_ = [
        ("submits", U64),
        ("waits", U64),
        ("busy", U64),
        ("max_inflight", U64),
        ("submit_ms", ctypes.c_double),
        ("wait_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BelowStats(ctypes.Structure):
    _fields_ = [
        ("calls", U64),
        ("slices", U64),
        ("sparse_slices", U64),
        ("dense_slices", U64),
        ("examined", U64),
        ("scan_nonces", U64),
        ("mark_nonces", U64),
        ("candidate_tiles", U64),
        ("mark_launches", U64),
        ("hits", U64),
        ("wall_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BelowRequest(ctypes.Structure):
    _fields_ = [("msg", ctypes.c_char_p), ("msg_len", ctypes.c_size_t), ("lower", U64), ("upper", U64),
                ("target", U64), ("cap", ctypes.c_size_t)]


class BelowBatchStats(ctypes.Structure):
    _fields_ = [
        ("calls", U64),
        ("requests", U64),
        ("empty", U64),
        ("coalesced", U64),
        ("individual", U64),
        ("rounds", U64),
        ("launches", U64),
        ("tiles", U64),
        ("mark_nonces", U64),
        ("hits", U64),
        ("bytes_back", U64),
        ("wall_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BelowWideStats(ctypes.Structure):
    _fields_ = [
        ("calls", U64),
        ("requests", U64),
        ("empty", U64),
        ("coalesced", U64),
        ("filtered", U64),
        ("individual", U64),
        ("rounds", U64),
        ("groups", U64),
        ("scan_launches", U64),
        ("scan_segments", U64),
        ("generic_launches", U64),
        ("scan_nonces", U64),
        ("filter_launches", U64),
        ("candidate_tiles", U64),
        ("slot_overflows", U64),
        ("mark_launches", U64),
        ("mark_tiles", U64),
        ("mark_nonces", U64),
        ("hits", U64),
        ("bytes_back", U64),
        ("wall_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DeviceInfo(ctypes.Structure):
    _fields_ = [
        ("ordinal", ctypes.c_int32),
        ("cu_count", ctypes.c_int32),
        ("clock_khz", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("hbm_bytes", U64),
        ("pci_bus_id", ctypes.c_char * 32),
        ("arch", ctypes.c_char * 32),
        ("uuid", ctypes.c_ubyte * 16),
    ]

    def as_dict(self):
        return {"ordinal": self.ordinal, "cu_count": self.cu_count, "clock_khz": self.clock_khz,
                "hbm_bytes": self.hbm_bytes, "pci_bus_id": self.pci_bus_id.decode(errors="replace"),
                "arch": self.arch.decode(errors="replace"), "uuid": bytes(self.uuid).hex()}


class TileRun(ctypes.Structure):
    _fields_ = [("first", U64), ("stride", U64), ("run_len", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class Tile(ctypes.Structure):
    _fields_ = [
        ("launch", ctypes.c_uint32),
        ("tile", ctypes.c_uint32),
        ("kind", ctypes.c_uint32),
        ("k", ctypes.c_uint32),
        ("nruns", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("runs", TileRun * 4),
        ("hash", U64),
        ("nonce", U64),
    ]


def lib_path():
    # P1HIP_LIB selects an alternative build of the same library (A/B tuning
    # builds under p1_amd/variants/); default is the in-tree libp1hip.so.
    return os.environ.get("P1HIP_LIB") or os.path.join(_HERE, "libp1hip.so")


# (name, restype, argtypes) for every entry point of include/p1hip.h
SIGNATURES = [
    ("p1hip_init", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    ("p1hip_init_devices", ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    ("p1hip_scan", ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_size_t, U64, U64, ctypes.POINTER(U64), ctypes.POINTER(U64)]),
    ("p1hip_scan_batch", ctypes.c_int, [ctypes.POINTER(Request), ctypes.c_size_t, ctypes.POINTER(Result)]),
    ("p1hip_batch_layout", ctypes.c_int,
     [ctypes.POINTER(Request), ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32),
      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    ("p1hip_get_batch_stats", ctypes.c_int, [ctypes.POINTER(BatchStats)]),
    ("p1hip_scan_batch_wide", ctypes.c_int, [ctypes.POINTER(Request), ctypes.c_size_t, ctypes.POINTER(Result)]),
    ("p1hip_wide_layout", ctypes.c_int,
     [ctypes.POINTER(Request), ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    ("p1hip_wide_ranges", ctypes.c_int,
     [ctypes.POINTER(Request), ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
      ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)]),
    ("p1hip_get_wide_stats", ctypes.c_int, [ctypes.POINTER(WideStats)]),
    ("p1hip_batch_submit", ctypes.c_int,
     [ctypes.POINTER(Request), ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(U64)]),
    ("p1hip_batch_wait", ctypes.c_int, [U64, ctypes.POINTER(Result)]),
    ("p1hip_get_async_stats", ctypes.c_int, [ctypes.POINTER(AsyncStats)]),
    ("p1hip_scan_below", ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_size_t, U64, U64, U64, ctypes.c_size_t, ctypes.POINTER(Result),
      ctypes.POINTER(ctypes.c_size_t)]),
    ("p1hip_get_below_stats", ctypes.c_int, [ctypes.POINTER(BelowStats)]),
    ("p1hip_scan_below_batch", ctypes.c_int,
     [ctypes.POINTER(BelowRequest), ctypes.c_size_t, ctypes.POINTER(Result), ctypes.c_size_t,
      ctypes.POINTER(ctypes.c_size_t)]),
    ("p1hip_below_batch_layout", ctypes.c_int,
     [ctypes.POINTER(BelowRequest), ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)]),
    ("p1hip_get_below_batch_stats", ctypes.c_int, [ctypes.POINTER(BelowBatchStats)]),
    ("p1hip_below_collect", ctypes.c_int,
     [ctypes.POINTER(U64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
      ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    ("p1hip_scan_below_batch_wide", ctypes.c_int,
     [ctypes.POINTER(BelowRequest), ctypes.c_size_t, ctypes.POINTER(Result), ctypes.c_size_t,
      ctypes.POINTER(ctypes.c_size_t)]),
    ("p1hip_below_wide_layout", ctypes.c_int,
     [ctypes.POINTER(BelowRequest), ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    ("p1hip_get_below_wide_stats", ctypes.c_int, [ctypes.POINTER(BelowWideStats)]),
    ("p1hip_below_filter", ctypes.c_int,
     [ctypes.POINTER(U64), ctypes.POINTER(U64), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
      ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(U64),
      ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
      ctypes.POINTER(ctypes.c_uint32)]),
    ("p1hip_hash", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, U64, ctypes.POINTER(U64)]),
    ("p1hip_plan_shards", ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_size_t, U64, U64, ctypes.c_int, ctypes.POINTER(U64), ctypes.POINTER(U64)]),
    ("p1hip_reduce_pairs", ctypes.c_int,
     [ctypes.POINTER(U64), ctypes.POINTER(U64), ctypes.c_size_t, ctypes.POINTER(U64), ctypes.POINTER(U64)]),
    ("p1hip_scan_tiles", ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_size_t, U64, U64, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
      ctypes.POINTER(Tile), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(U64), ctypes.POINTER(U64)]),
    ("p1hip_set_profiling", ctypes.c_int, [ctypes.c_int]),
    ("p1hip_get_stats", ctypes.c_int, [ctypes.POINTER(Stats)]),
    ("p1hip_reset_stats", None, []),
    ("p1hip_get_device_stats", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(DeviceStats)]),
    ("p1hip_device_count", ctypes.c_int, []),
    ("p1hip_device_info", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(DeviceInfo)]),
    ("p1hip_comm_info", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("p1hip_abi_version", ctypes.c_int, []),
    ("p1hip_test_knobs", ctypes.c_char_p, []),
    ("p1hip_last_error", ctypes.c_char_p, []),
    ("p1hip_version", ctypes.c_char_p, []),
    ("p1hip_shutdown", None, []),
]


def load(path=None):
    """Load libp1hip.so (once).  Raises if it is missing or incomplete."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or lib_path()
    if not os.path.exists(p):
        raise P1HipError(-100, f"{p} not built (run `make` or __graft_entry__.build())")
    lib = ctypes.CDLL(p)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.p1hip_abi_version() != ABI_VERSION:
        raise P1HipError(-100, f"{p}: ABI version {lib.p1hip_abi_version()}, this binding reads version "
                               f"{ABI_VERSION} structs (rebuild the library)")
    if path is None:
        _LIB = lib
    return lib


def _check(rc):
    if rc != 0:
        raise P1HipError(rc, load().p1hip_last_error().decode(errors="replace"))


def _bytes(msg):
    if isinstance(msg, str):
        return msg.encode("utf-8")  # Go strings are UTF-8 bytes after the JSON round trip
    return bytes(msg)


def init(want_devices=0):
    got = ctypes.c_int(0)
    _check(load().p1hip_init(int(want_devices), ctypes.byref(got)))
    return got.value


def init_devices(ordinals):
    arr = (ctypes.c_int * len(ordinals))(*ordinals)
    _check(load().p1hip_init_devices(arr, len(ordinals)))


def scan(msg, lower, upper):
    """miner.go:56-63 on the GPU: (min hash, its nonce) over [lower, upper]."""
    m = _bytes(msg)
    h, n = U64(), U64()
    _check(load().p1hip_scan(m, len(m), int(lower), int(upper), ctypes.byref(h), ctypes.byref(n)))
    return h.value, n.value


def _requests(requests):
    """(array of Request, the message bytes it borrows) for an iterable of
    (msg, lower, upper)."""
    rows = [(_bytes(m), int(lo), int(hi)) for m, lo, hi in requests]
    arr = (Request * max(len(rows), 1))()
    for r, (m, lo, hi) in zip(arr, rows):
        r.msg, r.msg_len, r.lower, r.upper = m, len(m), lo, hi
    return arr, rows


def scan_batch(requests):
    """p1hip_scan_batch: `requests` is an iterable of (msg, lower, upper), msg
    as for scan(); returns [(hash, nonce)] in request order, each exactly what
    scan(msg, lower, upper) returns.  Requests of at most 2^16 nonces share
    one launch pair per device instead of paying one launch each."""
    arr, rows = _requests(requests)
    out = (Result * max(len(rows), 1))()
    _check(load().p1hip_scan_batch(arr, len(rows), out))
    return [(out[i].hash, out[i].nonce) for i in range(len(rows))]


def batch_layout(requests, ndev):
    """p1hip_batch_layout: how scan_batch would lay `requests` out over `ndev`
    devices; one {"tiles", "device", "launch"} per request (tiles 0 and
    device / launch -1: empty range, or run individually).  Host-only."""
    arr, rows = _requests(requests)
    n = len(rows)
    tiles = (ctypes.c_uint32 * max(n, 1))()
    device = (ctypes.c_int32 * max(n, 1))()
    launch = (ctypes.c_int32 * max(n, 1))()
    _check(load().p1hip_batch_layout(arr, n, int(ndev), tiles, device, launch))
    return [{"tiles": tiles[i], "device": device[i], "launch": launch[i]} for i in range(n)]


def get_batch_stats():
    """Accounting of scan_batch since reset_stats (p1hip_get_batch_stats)."""
    s = BatchStats()
    _check(load().p1hip_get_batch_stats(ctypes.byref(s)))
    return s.as_dict()


WIDE_ROUTES = ("empty", "small", "wide", "individual")


def scan_batch_wide(requests):
    """p1hip_scan_batch_wide: as scan_batch, and the requests above 2^16 and
    of at most 2^24 nonces share k_scan launches instead of running alone."""
    arr, rows = _requests(requests)
    out = (Result * max(len(rows), 1))()
    _check(load().p1hip_scan_batch_wide(arr, len(rows), out))
    return [(out[i].hash, out[i].nonce) for i in range(len(rows))]


def wide_layout(requests, ndev):
    """p1hip_wide_layout + p1hip_wide_ranges: how scan_batch_wide would lay
    `requests` out over `ndev` devices.  Returns (per request {"route" (one
    of WIDE_ROUTES), "device", "segs", "tiles", "ranges": [(tile0, ntiles,
    launch)]}, [tiles of each device's partial array]); a range's launch is
    the device's k_scan launch that writes it, -1 for the generic tiles.
    Host-only."""
    arr, rows = _requests(requests)
    n = len(rows)
    route, device = (ctypes.c_int32 * max(n, 1))(), (ctypes.c_int32 * max(n, 1))()
    segs, tiles = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
    _check(load().p1hip_wide_layout(arr, n, int(ndev), route, device, segs, tiles))
    lay = [{"route": WIDE_ROUTES[route[i]], "device": device[i], "segs": segs[i], "tiles": tiles[i], "ranges": []}
           for i in range(n)]
    cap = sum(x["segs"] + 1 for x in lay)  # one range per segment, one for the generic tiles
    count = ctypes.c_size_t(0)
    req, tile0, ntiles = ((ctypes.c_uint32 * max(cap, 1))() for _ in range(3))
    launch = (ctypes.c_int32 * max(cap, 1))()
    dev_tiles = (ctypes.c_uint32 * int(ndev))()
    _check(load().p1hip_wide_ranges(arr, n, int(ndev), cap, ctypes.byref(count), req, tile0, ntiles, launch,
                                    dev_tiles))
    assert count.value <= cap
    for j in range(count.value):
        lay[req[j]]["ranges"].append((tile0[j], ntiles[j], launch[j]))
    return lay, list(dev_tiles)


def get_wide_stats():
    """Accounting of scan_batch_wide since reset_stats (p1hip_get_wide_stats)."""
    s = WideStats()
    _check(load().p1hip_get_wide_stats(ctypes.byref(s)))
    return s.as_dict()


# include/p1hip.h P1HIP_ERR_BUSY, P1HIP_MAX_INFLIGHT
ERR_BUSY = -5
MAX_INFLIGHT = 4
_TICKET_SIZES = {}  # ticket -> number of requests (batch_wait sizes its result array by it)


def batch_submit(requests, wide=False):
    """p1hip_batch_submit: enqueue the call scan_batch (or, with `wide`,
    scan_batch_wide) would make of `requests` and return its ticket at once,
    without waiting for the device.  At most MAX_INFLIGHT tickets may be
    outstanding: one more raises P1HipError with rc == ERR_BUSY."""
    arr, rows = _requests(requests)
    t = U64(0)
    _check(load().p1hip_batch_submit(arr, len(rows), 1 if wide else 0, ctypes.byref(t)))
    _TICKET_SIZES[t.value] = len(rows)
    return t.value


def batch_wait(ticket):
    """p1hip_batch_wait: block until `ticket`'s call is done; [(hash, nonce)]
    in request order, each exactly what scan(msg, lower, upper) returns.  The
    ticket is spent afterwards, on success and on error alike."""
    n = _TICKET_SIZES.pop(int(ticket), 0)
    out = (Result * max(n, 1))()
    _check(load().p1hip_batch_wait(int(ticket), out))
    return [(out[i].hash, out[i].nonce) for i in range(n)]


def get_async_stats():
    """Accounting of batch_submit / batch_wait since reset_stats."""
    s = AsyncStats()
    _check(load().p1hip_get_async_stats(ctypes.byref(s)))
    return s.as_dict()


# include/p1hip.h P1HIP_BELOW_MAX_SLICE, P1HIP_BELOW_MAX_SLICE_DENSE, P1HIP_BELOW_DENSE_TARGET
BELOW_MAX_SLICE = 1 << 34
BELOW_MAX_SLICE_DENSE = 1 << 28
BELOW_DENSE_TARGET = 1 << 46


def scan_below(msg, lower, upper, target, cap=1):
    """p1hip_scan_below: [(hash, nonce)] of the nonces n of [lower, upper] with
    bitcoin.Hash(msg, n) <= target, in increasing n, the first `cap` of them.
    Fewer than `cap`: these are all hits of the range; exactly `cap`: there
    may be more, resume with lower = the last nonce + 1."""
    m = _bytes(msg)
    cap = int(cap)
    out = (Result * max(cap, 1))()
    found = ctypes.c_size_t(0)
    _check(load().p1hip_scan_below(m, len(m), int(lower), int(upper), int(target), cap, out, ctypes.byref(found)))
    return [(out[i].hash, out[i].nonce) for i in range(found.value)]


def get_below_stats():
    """Accounting of scan_below since reset_stats (p1hip_get_below_stats)."""
    s = BelowStats()
    _check(load().p1hip_get_below_stats(ctypes.byref(s)))
    return s.as_dict()


# include/p1hip.h P1HIP_BELOW_BATCH_MAX_NONCES, P1HIP_BELOW_BATCH_MAX_SLOTS
BELOW_BATCH_MAX_NONCES = 1 << 20
BELOW_BATCH_MAX_SLOTS = 1 << 22
BELOW_BATCH_ROUTES = ("empty", "coalesced", "individual")


def _below_requests(requests):
    """(array of BelowRequest, the rows it borrows its messages from) for an
    iterable of (msg, lower, upper, target, cap)."""
    rows = [(_bytes(m), int(lo), int(hi), int(t), int(cap)) for m, lo, hi, t, cap in requests]
    arr = (BelowRequest * max(len(rows), 1))()
    for r, (m, lo, hi, t, cap) in zip(arr, rows):
        r.msg, r.msg_len, r.lower, r.upper, r.target, r.cap = m, len(m), lo, hi, t, cap
    return arr, rows


def scan_below_batch(requests):
    """p1hip_scan_below_batch: `requests` is an iterable of (msg, lower, upper,
    target, cap); returns one list per request, in order, each exactly what
    scan_below(msg, lower, upper, target, cap) returns.  The requests whose
    slices are dense and of at most 2^20 nonces share launch pairs."""
    arr, rows = _below_requests(requests)
    n = len(rows)
    total = sum(r[4] for r in rows)
    hits = (Result * max(total, 1))()
    found = (ctypes.c_size_t * max(n, 1))()
    _check(load().p1hip_scan_below_batch(arr, n, hits, total, found))
    out, off = [], 0
    for i in range(n):
        out.append([(hits[off + k].hash, hits[off + k].nonce) for k in range(found[i])])
        off += rows[i][4]
    return out


def below_batch_layout(requests, ndev):
    """p1hip_below_batch_layout: per request {"route" (one of
    BELOW_BATCH_ROUTES), "device", "tiles"} of scan_below_batch's first round
    over `ndev` devices (device -1 and tiles 0 unless coalesced).  Host-only."""
    arr, rows = _below_requests(requests)
    n = len(rows)
    route, device = (ctypes.c_int32 * max(n, 1))(), (ctypes.c_int32 * max(n, 1))()
    tiles = (ctypes.c_uint32 * max(n, 1))()
    _check(load().p1hip_below_batch_layout(arr, n, int(ndev), route, device, tiles))
    return [{"route": BELOW_BATCH_ROUTES[route[i]], "device": device[i], "tiles": tiles[i]} for i in range(n)]


def get_below_batch_stats():
    """Accounting of scan_below_batch since reset_stats (p1hip_get_below_batch_stats)."""
    s = BelowBatchStats()
    _check(load().p1hip_get_below_batch_stats(ctypes.byref(s)))
    return s.as_dict()


def below_collect(words, req_tile0, req_hit0):
    """p1hip_below_collect (test hook): k_belowb_collect alone over the mark
    words `words`; request r owns words [4 * req_tile0[r], 4 * req_tile0[r + 1])
    and slots [req_hit0[r], req_hit0[r + 1]).  Returns (idx, count): every slot
    (UINT32_MAX where the kernel wrote nothing) and the hits per request."""
    nreq = len(req_tile0) - 1
    assert nreq >= 0 and len(req_hit0) == nreq + 1 and len(words) == 4 * req_tile0[-1]
    wa = (U64 * max(len(words), 1))(*words)
    ta = (ctypes.c_uint32 * (nreq + 1))(*req_tile0)
    ha = (ctypes.c_uint32 * (nreq + 1))(*req_hit0)
    idx = (ctypes.c_uint32 * max(req_hit0[-1], 1))()
    count = (ctypes.c_uint32 * max(nreq, 1))()
    _check(load().p1hip_below_collect(wa, ta, ha, nreq, idx, count))
    return list(idx[:req_hit0[-1]]), list(count[:nreq])


def belowb_codeobj_sha256(lib=None):
    """sha256 (hex) of the fourth embedded code object, the kernels of
    scan_below_batch (p1hip_belowb_co .. p1hip_belowb_co_end of
    csrc/p1hip_belowb_blob.S)."""
    import hashlib

    lib = lib or load()
    start = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_belowb_co"))
    end = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_belowb_co_end"))
    if end <= start:
        raise P1HipError(-100, "embedded below batch code object is empty")
    return hashlib.sha256(ctypes.string_at(start, end - start)).hexdigest()


# include/p1hip.h P1HIP_BELOW_WIDE_MAX_NONCES; route[i] of p1hip_below_wide_layout
BELOW_WIDE_MAX_NONCES = 1 << 24
BELOW_WIDE_ROUTES = ("empty", "coalesced", "individual", "filtered")


def scan_below_batch_wide(requests):
    """p1hip_scan_below_batch_wide: scan_below_batch's contract and result;
    the requests whose first slice is sparse and of at most 2^24 nonces (hard
    targets) share k_scan launches and a filter kernel instead of running one
    by one."""
    arr, rows = _below_requests(requests)
    n = len(rows)
    total = sum(r[4] for r in rows)
    hits = (Result * max(total, 1))()
    found = (ctypes.c_size_t * max(n, 1))()
    _check(load().p1hip_scan_below_batch_wide(arr, n, hits, total, found))
    out, off = [], 0
    for i in range(n):
        out.append([(hits[off + k].hash, hits[off + k].nonce) for k in range(found[i])])
        off += rows[i][4]
    return out


def below_wide_layout(requests, ndev):
    """p1hip_below_wide_layout: per request {"route" (one of BELOW_WIDE_ROUTES),
    "device", "tiles", "slots"} of scan_below_batch_wide's first round over
    `ndev` devices (device -1, tiles and slots 0 unless coalesced or filtered).
    Host-only."""
    arr, rows = _below_requests(requests)
    n = len(rows)
    route, device = (ctypes.c_int32 * max(n, 1))(), (ctypes.c_int32 * max(n, 1))()
    tiles, slots = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
    _check(load().p1hip_below_wide_layout(arr, n, int(ndev), route, device, tiles, slots))
    return [{"route": BELOW_WIDE_ROUTES[route[i]], "device": device[i], "tiles": tiles[i], "slots": slots[i]}
            for i in range(n)]


def get_below_wide_stats():
    """Accounting of scan_below_batch_wide since reset_stats (p1hip_get_below_wide_stats)."""
    s = BelowWideStats()
    _check(load().p1hip_get_below_wide_stats(ctypes.byref(s)))
    return s.as_dict()


def below_filter(part, ranges, req_range0, targets, req_slot0):
    """p1hip_below_filter (test hook): k_beloww_filter alone over the partial
    array `part` [(hash, nonce)]; `ranges` is [(tile0, ntiles)], request r owns
    ranges [req_range0[r], req_range0[r + 1]) and slots [req_slot0[r],
    req_slot0[r + 1]).  Returns (cand, count): every slot (UINT32_MAX where
    the kernel wrote nothing) and the candidates of each request, not clamped."""
    nreq = len(req_range0) - 1
    assert nreq >= 0 and len(req_slot0) == nreq + 1 and len(targets) == nreq and len(ranges) == req_range0[-1]
    nt = len(part)
    ha = (U64 * max(nt, 1))(*[h for h, _ in part])
    na = (U64 * max(nt, 1))(*[x for _, x in part])
    t0 = (ctypes.c_uint32 * max(len(ranges), 1))(*[a for a, _ in ranges])
    tn = (ctypes.c_uint32 * max(len(ranges), 1))(*[b for _, b in ranges])
    ra = (ctypes.c_uint32 * (nreq + 1))(*req_range0)
    sa = (ctypes.c_uint32 * (nreq + 1))(*req_slot0)
    ta = (U64 * max(nreq, 1))(*targets)
    cand = (ctypes.c_uint32 * max(req_slot0[-1], 1))()
    count = (ctypes.c_uint32 * max(nreq, 1))()
    _check(load().p1hip_below_filter(ha, na, nt, t0, tn, ra, ta, sa, nreq, cand, count))
    return list(cand[:req_slot0[-1]]), list(count[:nreq])


def beloww_codeobj_sha256(lib=None):
    """sha256 (hex) of the fifth embedded code object, the filter kernel of
    scan_below_batch_wide (p1hip_beloww_co .. p1hip_beloww_co_end of
    csrc/p1hip_beloww_blob.S)."""
    import hashlib

    lib = lib or load()
    start = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_beloww_co"))
    end = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_beloww_co_end"))
    if end <= start:
        raise P1HipError(-100, "embedded below wide code object is empty")
    return hashlib.sha256(ctypes.string_at(start, end - start)).hexdigest()


def below_codeobj_sha256(lib=None):
    """sha256 (hex) of the third embedded code object, the mark kernel of
    scan_below (p1hip_below_co .. p1hip_below_co_end of csrc/p1hip_below_blob.S)."""
    import hashlib

    lib = lib or load()
    start = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_below_co"))
    end = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_below_co_end"))
    if end <= start:
        raise P1HipError(-100, "embedded below code object is empty")
    return hashlib.sha256(ctypes.string_at(start, end - start)).hexdigest()


def batch_codeobj_sha256(lib=None):
    """sha256 (hex) of the second embedded code object, the batch kernels
    (p1hip_batch_co .. p1hip_batch_co_end of csrc/p1hip_batch_blob.S)."""
    import hashlib

    lib = lib or load()
    start = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_batch_co"))
    end = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_batch_co_end"))
    if end <= start:
        raise P1HipError(-100, "embedded batch code object is empty")
    return hashlib.sha256(ctypes.string_at(start, end - start)).hexdigest()


def hash(msg, nonce):  # noqa: A001 - mirrors bitcoin.Hash
    m = _bytes(msg)
    h = U64()
    _check(load().p1hip_hash(m, len(m), int(nonce), ctypes.byref(h)))
    return h.value


def plan_shards(msg, lower, upper, n):
    """p1hip_plan_shards: [lower, upper] cut into n contiguous shards of
    near-equal predicted GPU time; a list of inclusive (lo, hi) or None for
    an empty shard.  Host-only: needs the library, not a device."""
    m = _bytes(msg)
    first, last = (U64 * n)(), (U64 * n)()
    _check(load().p1hip_plan_shards(m, len(m), int(lower), int(upper), int(n), first, last))
    return [(a, b) if a <= b else None for a, b in zip(first, last)]


def reduce_pairs(hashes, nonces):
    n = len(hashes)
    assert n == len(nonces)
    ha = (U64 * max(n, 1))(*hashes)
    na = (U64 * max(n, 1))(*nonces)
    h, o = U64(), U64()
    _check(load().p1hip_reduce_pairs(ha, na, n, ctypes.byref(h), ctypes.byref(o)))
    return h.value, o.value


# include/p1hip.h P1HIP_TILE_POISON as a partial reads when no tile wrote it
TILE_POISON = int.from_bytes(b"\xa5" * 8, "little")
TILE_GENERIC_KIND = 255
TILE_ROUTES = ("scan", "small")


def scan_tiles(msg, lower, upper):
    """p1hip_scan_tiles (test hook): one scan of [lower, upper] on the first
    device with its partials poisoned first and read back raw.  Returns
    (route ("scan" or "small"), tiles, (hash, nonce)): tiles in partial-array
    order, each (launch, tile, kind, k, (hash, nonce), runs) with runs a list
    of (first, run_len, stride, count) -- the layout tools/p1emu's `tiles`
    lines parse to (tests/tile_check.py)."""
    m = _bytes(msg)
    lib = load()
    count, route = ctypes.c_size_t(0), ctypes.c_int(-1)
    h, n = U64(), U64()
    # the tiles of a range are at most one per 256 nonces, one more per piece
    # (ragged last tile), and the padded waves of MODE 5; ask again if short
    cap = min(max(int(upper) - int(lower), 0) // 256 + 64, 1 << 20)
    while True:
        arr = (Tile * cap)()
        _check(lib.p1hip_scan_tiles(m, len(m), int(lower), int(upper), cap, ctypes.byref(count), arr,
                                    ctypes.byref(route), ctypes.byref(h), ctypes.byref(n)))
        if count.value <= cap:
            break
        cap = count.value
    tiles = [(t.launch, t.tile, t.kind, t.k, (t.hash, t.nonce),
              [(r.first, r.run_len, r.stride, r.count) for r in t.runs[:t.nruns]]) for t in arr[:count.value]]
    return TILE_ROUTES[route.value], tiles, (h.value, n.value)


def set_profiling(on):
    _check(load().p1hip_set_profiling(1 if on else 0))


def get_stats():
    s = Stats()
    _check(load().p1hip_get_stats(ctypes.byref(s)))
    return s.as_dict()


def get_device_stats(index):
    """Per-device accounting since reset_stats (p1hip_get_device_stats)."""
    s = DeviceStats()
    _check(load().p1hip_get_device_stats(int(index), ctypes.byref(s)))
    return s.as_dict()


def device_info(index):
    """Identity of device `index` (p1hip_device_info): ordinal, PCI bus id,
    arch, CU count, clock, HBM bytes, UUID."""
    s = DeviceInfo()
    _check(load().p1hip_device_info(int(index), ctypes.byref(s)))
    return s.as_dict()


def comm_info(index):
    """(nranks, rank) of device `index`'s RCCL communicator as RCCL reports
    it (p1hip_comm_info: ncclCommCount / ncclCommUserRank); (0, -1) for a
    device without one."""
    n, r = ctypes.c_int(0), ctypes.c_int(-1)
    _check(load().p1hip_comm_info(int(index), ctypes.byref(n), ctypes.byref(r)))
    return n.value, r.value


# include/p1hip.h P1HIP_ABI_VERSION: the struct layouts this module declares
ABI_VERSION = 6


def abi_version():
    return load().p1hip_abi_version()


def test_knobs():
    """The library's test knobs in force for this process, as a dict ({} in
    production: the knobs are honoured only under P1HIP_TEST_KNOBS=1)."""
    raw = load().p1hip_test_knobs().decode()
    return dict(kv.split("=", 1) if "=" in kv else (kv, "?") for kv in raw.split(";") if kv)


def reset_stats():
    load().p1hip_reset_stats()


def device_count():
    return load().p1hip_device_count()


def shutdown():
    load().p1hip_shutdown()


def version():
    return load().p1hip_version().decode()


def codeobj_bytes(lib=None):
    """The gfx950 code object embedded in the library (the bytes between the
    p1hip_kernels_co / p1hip_kernels_co_end symbols of
    csrc/p1hip_kernels_blob.S, i.e. build/p1hip_kernels.hsaco as linked):
    the exact kernels every scan through this library runs."""
    lib = lib or load()
    start = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_kernels_co"))
    end = ctypes.addressof(ctypes.c_char.in_dll(lib, "p1hip_kernels_co_end"))
    if end <= start:
        raise P1HipError(-100, "embedded code object is empty")
    return ctypes.string_at(start, end - start)


def codeobj_sha256(lib=None):
    """sha256 (hex) of the embedded code object: the key that ties a rocprof
    or PMC summary under profiles/ to the kernels it measured."""
    import hashlib

    return hashlib.sha256(codeobj_bytes(lib)).hexdigest()
