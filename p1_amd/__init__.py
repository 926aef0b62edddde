"""p1_amd -- MI355X (gfx950) drop-in for the bitcoin miner's nonce scan.

The product is the C-ABI library ``p1_amd/libp1hip.so`` (include/p1hip.h).
This package is thin Python plumbing over it (ctypes), used by bench.py and
the tests.  There is no CPU fallback: every call goes to the HIP kernels and
raises if the library or a gfx950 device is missing.

Reference seam: /root/reference/src/github.com/cmu440/bitcoin/miner/miner.go:56-63.
"""
from ._lib import (  # noqa: F401
    P1HipError,
    lib_path,
    load,
    init,
    init_devices,
    scan,
    scan_batch,
    batch_layout,
    get_batch_stats,
    scan_batch_wide,
    wide_layout,
    get_wide_stats,
    batch_submit,
    batch_wait,
    get_async_stats,
    ERR_BUSY,
    MAX_INFLIGHT,
    hash,
    reduce_pairs,
    scan_tiles,
    TILE_POISON,
    TILE_GENERIC_KIND,
    plan_shards,
    set_profiling,
    get_stats,
    get_device_stats,
    reset_stats,
    device_count,
    device_info,
    comm_info,
    abi_version,
    ABI_VERSION,
    test_knobs,
    shutdown,
    version,
    codeobj_bytes,
    codeobj_sha256,
    batch_codeobj_sha256,
    scan_below,
    get_below_stats,
    below_codeobj_sha256,
    BELOW_MAX_SLICE,
    BELOW_MAX_SLICE_DENSE,
    BELOW_DENSE_TARGET,
    scan_below_batch,
    below_batch_layout,
    get_below_batch_stats,
    below_collect,
    belowb_codeobj_sha256,
    BELOW_BATCH_MAX_NONCES,
    BELOW_BATCH_MAX_SLOTS,
    BELOW_BATCH_ROUTES,
)
from .sharding import shard_range, combine_keys  # noqa: F401
