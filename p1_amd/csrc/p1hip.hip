// p1hip.hip -- libp1hip.so: host runtime (planning, launch orchestration,
// multi-device combine) and the C ABI declared in include/p1hip.h.
//
// Replaces the miner's scan loop /root/reference/src/github.com/cmu440/bitcoin/
// miner/miner.go:56-63 (see include/p1hip.h for the exact contract).
//
// Device pipeline of one p1hip_scan on one device (one HIP stream):
//   planner.hpp   -> list of pieces (fast: one thread per 10^k nonces;
//                    generic: one thread per nonce, for ragged edges)
//   scan_pack.hpp -> the pieces ordered and cut into launches, one segment
//                    table per launch (host only; tools/p1emu replays it)
//   k_scan        -> one launch, one segment per piece (p1hip_kernels.hip)
//   k_reduce      -> one workgroup folds all partials into the device result
// The kernels live in a gfx950 code object built from p1hip_kernels.hip via
// assembly + tools/isa_post.py (Makefile) and embedded in this library
// (p1hip_kernels_blob.S); each device loads it with hipModuleLoadData.
// Several devices: contiguous shards, one host thread per device, RCCL
// all-gather of the 16-byte results (ncclCommInitAll), host lexicographic min.
//
// p1hip_scan_batch: many small requests (of any messages) in one launch pair
// per device, k_batch_scan + k_batch_reduce, from a second, small code object
// (p1hip_batch_kernels.hip, p1hip_batch_blob.S); layout and tables come from
// batch_plan.hpp, which tools/batch_emu shares.
//
// p1hip_scan_batch_wide: the requests of a call above the batch limit and of
// at most 2^24 nonces share k_scan launches (the scan object's kernel, up to
// kMaxSegs segments of any messages per launch), their generic pieces one
// k_batch_scan launch, and k_wide_reduce (batch object) folds one result per
// request; the layout comes from wide_plan.hpp, which tools/batch_emu shares.
//
// p1hip_batch_submit / p1hip_batch_wait: the same two calls without the
// synchronisation.  submit enqueues the call in the buffers of one of
// P1HIP_MAX_INFLIGHT slots (SlotDev; tickets: async_slots.hpp) and records an
// event per device; wait blocks on the events with the runtime mutex released.
// Still one stream per device: k_scan's work-queue ticket is shared.
//
// p1hip_scan_below: every nonce whose hash is at or below a target, slice by
// slice.  A sparse slice runs the scan path's own run_range on every device
// and keeps the tiles whose partial is at or below the target; k_below_mark
// (a third code object, p1hip_below_kernels.hip, p1hip_below_blob.S) answers
// one bit per nonce of those tiles, or of the whole slice when it is dense.
// Slices, filter, tables and decoder come from below_plan.hpp, which
// tools/p1emu shares.
//
// p1hip_scan_below_batch: many target searches in one call.  The requests
// whose slices are dense and of at most 2^20 nonces advance in rounds; a round
// lays the current slice of each over the devices and launch pairs,
// k_belowb_mark marks them against each request's own target and
// k_belowb_collect turns the marks into hit indices on the device (a fourth
// code object, p1hip_belowb_kernels.hip, p1hip_belowb_blob.S).  Routes, round
// layout, tables and decoder come from belowb_plan.hpp, which tools/batch_emu
// shares.
//
// p1hip_scan_below_batch_wide: the same call with a third route.  The requests
// whose first slice is sparse and of at most 2^24 nonces share k_scan launches
// as the wide path's requests do; k_beloww_filter (a fifth code object,
// p1hip_beloww_kernels.hip, p1hip_beloww_blob.S) turns each request's partials
// into candidate tile indices on the device, and k_belowb_mark refines all
// candidates of a device in one launch.  Routes, round items, groups, the slot
// rule, tables and decoder come from beloww_plan.hpp, which tools/batch_emu
// shares.
//
// Order of this file: runtime state, helpers, the scan path, the batch path,
// the wide path, submit / wait, reduce_pairs, scan_tiles, scan_below,
// scan_below_batch, scan_below_batch_wide, then the C ABI in one extern "C" block.  Every HIP and RCCL
// call of the library is in this file (tests/test_stream_discipline.py).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/p1hip.h"
#include "async_slots.hpp"
#include "batch_plan.hpp"
#include "below_plan.hpp"
#include "belowb_plan.hpp"
#include "beloww_plan.hpp"
#include "planner.hpp"
#include "scan_abi.hpp"
#include "scan_pack.hpp"
#include "tile_map.hpp"
#include "wide_plan.hpp"

// the embedded gfx950 code objects (p1hip_kernels_blob.S, p1hip_batch_blob.S,
// p1hip_below_blob.S, p1hip_belowb_blob.S, p1hip_beloww_blob.S)
extern "C" const unsigned char p1hip_kernels_co[];
extern "C" const unsigned char p1hip_batch_co[];
extern "C" const unsigned char p1hip_below_co[];
extern "C" const unsigned char p1hip_belowb_co[];
extern "C" const unsigned char p1hip_beloww_co[];

using namespace p1;

namespace {

// ----------------------------------------------------------------------------
// Errors
// ----------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int rc, const std::string& what) {
  g_err = what;
  return rc;
}

// Run an exported entry point's body; a host exception (std::bad_alloc from a
// caller-sized allocation, std::system_error from a thread) becomes rc -2
// with the message in p1hip_last_error() instead of crossing the C ABI.
template <typename Fn>
int guarded(Fn&& fn) {
  try {
    return fn();
  } catch (const std::exception& ex) {
    return fail(P1HIP_ERR_HIP, std::string("host: ") + ex.what());
  } catch (...) {
    return fail(P1HIP_ERR_HIP, "host: unknown exception");
  }
}

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(P1HIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

#define NCCLCHK(expr)                                                                       \
  do {                                                                                      \
    ncclResult_t r_ = (expr);                                                               \
    if (r_ != ncclSuccess)                                                                  \
      return fail(P1HIP_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(r_));      \
  } while (0)

// ----------------------------------------------------------------------------
// Limits and test knobs
// ----------------------------------------------------------------------------
// Device copies of MODE 5 K+W tables are cached, at most this many ...
constexpr size_t kMaxKwTabs = 8;
// ... and at most this many bytes of them (a 7-digit table is 2.56 GB; one
// scan needs at most one table per MODE 5 decade, < 2.9 GB in all)
constexpr uint64_t kMaxKwTabBytes = 8ull << 30;
// A device's share runs in pieces of at most this many nonces (run_share).
constexpr uint64_t kMaxScanSpan = 1ull << 40;

// Every P1HIP_* test knob, in the order p1hip_test_knobs() lists them.  A knob
// is honoured only while the master switch P1HIP_TEST_KNOBS=1 is set (the
// test fixtures set it), so a stray knob in a production miner's environment
// changes nothing; bench.py refuses to time with any in force.  All are read
// through knob(): unset or empty gives `def`; a kFlag is on when its value
// starts with '1'; a number above `max` becomes `max`; 0 is a real 0 for
// kValue and means `def` for kZeroDef.
enum KnobKind { kValue, kZeroDef, kFlag };
enum KnobWhen { kPerScan, kPerBatch, kAtInit };  // init: the open devices keep what they were opened with
enum KnobId {
  kSmallMaxNoncesKnob, kMaxLaunchBlocksKnob, kMaxScanSpanKnob, kKwtabMaxBytesKnob, kNoRcclKnob, kForceRcclKnob,
  kMinFastThreadsKnob, kTestFailDeviceKnob, kNoTableKnob, kNoSplitKnob, kScanGridKnob, kBatchMaxNoncesKnob,
  kBatchMaxTilesKnob, kWideMaxNoncesKnob, kWideMaxSegsKnob, kWideMinFastThreadsKnob, kBelowPathKnob,
  kBelowMaxSliceKnob, kBelowWideMaxSlotsKnob, kKnobCount
};
struct Knob {
  const char* name;
  uint64_t def, max;
  KnobKind kind;
  KnobWhen when;
  const char* what;
};
const Knob kKnobs[] = {
    {"P1HIP_SMALL_MAX_NONCES", kSmallMaxNonces, kSmallMaxNonces, kValue, kPerScan,
     "shares of at most this many nonces take the one-launch small path; 0 turns it off, so small parity ranges "
     "run the fast kernel variants"},
    {"P1HIP_MAX_LAUNCH_BLOCKS", kMaxLaunchBlocks, kMaxLaunchBlocks, kZeroDef, kPerScan,
     "workgroups per k_scan launch, so GPU tests run the multi-launch path on small ranges; a larger piece gets "
     "a launch of its own (at most kMaxFastThreads / kBlock = 2^18 workgroups, far below HIP's grid limit)"},
    {"P1HIP_MAX_SCAN_SPAN", kMaxScanSpan, ~0ull, kZeroDef, kPerScan, "nonces per piece of a device's share"},
    {"P1HIP_KWTAB_MAX_BYTES", kMaxKwTabBytes, ~0ull, kValue, kPerScan,
     "MODE 5 table cap; a larger table re-plans the share without MODE 5"},
    {"P1HIP_NO_RCCL", 0, 1, kFlag, kAtInit,
     "combine the per-device results through the host, so the multi-device path (threads, sharding, combine) "
     "runs with the same GPU listed twice on a 1-GPU box"},
    {"P1HIP_FORCE_RCCL", 0, 1, kFlag, kAtInit, "a communicator even for one device"},
    {"P1HIP_MIN_FAST_THREADS", kMinFastThreads, ~0ull, kValue, kAtInit,
     "planner occupancy floor; 1 keeps k = 3 on small ranges so every k = 3 variant runs on the GPU"},
    {"P1HIP_TEST_FAIL_DEVICE", ~0ull, ~0ull, kValue, kAtInit,
     "device index whose scan phase reports a failure (the multi-device error path); default -1: none"},
    {"P1HIP_NO_TABLE", 0, 1, kFlag, kAtInit,
     "no MODE 5: layouts whose tail block 1 holds only lo digits run the digit-update variants (A/B, and a "
     "second kernel path to cross-check MODE 5)"},
    {"P1HIP_NO_SPLIT", 0, 1, kFlag, kAtInit,
     "straddling lo digits use mode 2 instead of the split modes (A/B builds with -DP1_NV2_PLAIN)"},
    {"P1HIP_SCAN_GRID", 0, kMaxLaunchBlocks, kZeroDef, kPerScan,
     "k_scan's grid instead of the device's workgroup slots (the default, 0); at or above a launch's tile count "
     "every workgroup runs one tile and the queue hands out none (the round-5 dispatch, same code object)"},
    {"P1HIP_BATCH_MAX_NONCES", kBatchMaxNonces, kBatchMaxNonces, kValue, kPerBatch,
     "requests of at most this many nonces are coalesced by p1hip_scan_batch; 0 runs every request "
     "individually; independent of P1HIP_SMALL_MAX_NONCES"},
    {"P1HIP_BATCH_MAX_TILES", kBatchMaxTiles, kBatchMaxTiles, kZeroDef, kPerBatch,
     "tiles per launch pair, so GPU tests run several launch pairs on small batches (batch_layout raises it to "
     "the largest single request's tile count)"},
    {"P1HIP_WIDE_MAX_NONCES", kWideMaxNonces, kWideMaxNonces, kValue, kPerBatch,
     "requests above the coalescing limit and of at most this many nonces share k_scan launches in "
     "p1hip_scan_batch_wide; larger ones run individually (0: all of them)"},
    {"P1HIP_WIDE_MAX_SEGS", kMaxSegs, kMaxSegs, kZeroDef, kPerBatch,
     "segments per k_scan launch of p1hip_scan_batch_wide, so GPU tests run many launches back to back on small "
     "calls and requests whose pieces land in different launches"},
    {"P1HIP_WIDE_MIN_FAST_THREADS", 0, ~0ull, kZeroDef, kPerBatch,
     "occupancy floor the wide requests are planned with instead of wide_min_fast_threads' rule (the default, "
     "0); 1 keeps k = 3"},
    {"P1HIP_BELOW_PATH", kBelowAuto, kBelowDense, kValue, kPerScan,
     "route of every slice of p1hip_scan_below: 0 chosen from the target (the default), 1 sparse (k_scan filters, "
     "the surviving tiles are marked), 2 dense (every nonce is marked), so GPU tests run both on one range"},
    {"P1HIP_BELOW_MAX_SLICE", 0, ~0ull, kZeroDef, kPerScan,
     "nonces per slice of p1hip_scan_below at the most, below the route's own limit, so GPU tests run several "
     "slices, with hits next to their edges, on small ranges"},
    {"P1HIP_BELOW_WIDE_MAX_SLOTS", 0, ~0ull, kZeroDef, kPerBatch,
     "candidate slots per request and round of p1hip_scan_below_batch_wide at the most, below the slot rule's own "
     "number (the default, 0), so GPU tests reach the host filter that answers a request with more candidates"},
};
static_assert(sizeof kKnobs / sizeof kKnobs[0] == kKnobCount, "one row per KnobId, in its order");

bool test_knobs_on() {
  const char* m = getenv("P1HIP_TEST_KNOBS");
  return m && m[0] == '1' && m[1] == 0;
}

// the knob's text if it is in force, else null
const char* test_knob(const char* name) {
  if (!test_knobs_on()) return nullptr;
  const char* v = getenv(name);
  return v && *v ? v : nullptr;
}

uint64_t knob(KnobId id) {
  const Knob& K = kKnobs[id];
  const char* v = test_knob(K.name);
  if (!v) return K.def;
  if (K.kind == kFlag) return v[0] == '1';
  const uint64_t n = strtoull(v, nullptr, 10);
  if (n == 0 && K.kind == kZeroDef) return K.def;
  return n < K.max ? n : K.max;
}

// ----------------------------------------------------------------------------
// Runtime state
// ----------------------------------------------------------------------------
// A device (hipMalloc) or pinned host (hipHostMalloc) array that grows by
// powers of two and is kept.  It frees what it holds when it is destroyed or
// assigned over, so whoever does that has the owning device current and its
// stream synchronised (dev_release; reduce_pairs_locked's locals).
template <typename T, bool kPinned>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;  // elements `reserve` promised (`extra` more are allocated)

  Buf() = default;
  Buf(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      (void)release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~Buf() { (void)release(); }

  hipError_t release() {
    hipError_t e = hipSuccess;
    if (p) e = kPinned ? hipHostFree(p) : hipFree(p);
    p = nullptr;  // never a dangling pointer with a stale capacity
    cap = 0;
    return e;
  }
  // Room for `need` elements: if there is less, free, then allocate the next
  // power-of-two multiple of `floor` at or above `need` (+ `extra`).  Only
  // while the stream is idle.  On failure the buffer is empty.
  hipError_t reserve(size_t need, size_t floor, size_t extra = 0) {
    if (need <= cap) return hipSuccess;
    hipError_t e = release();
    if (e != hipSuccess) return e;
    size_t n = floor;
    while (n < need) n <<= 1;
    const size_t bytes = (n + extra) * sizeof(T);
    e = kPinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess) p = nullptr;
    else cap = n;
    return e;
  }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

// One device's buffers of one p1hip_batch_submit slot: everything a ticket's
// launches read or write on this device, so that the next submit (another
// slot) and the synchronous calls (the Dev's own buffers) never touch what an
// outstanding ticket still uses.  The small and the wide route of one call
// run back to back without a synchronisation, so they share nothing either.
// Grown only by the submit that has just taken the slot, i.e. while it is idle.
struct SlotDev {
  // small route: every launch pair of the call at its own offset
  DevBuf<BatchSeg> d_bseg;
  PinnedBuf<BatchSeg> h_bseg;
  DevBuf<uint32_t> d_btile0;
  PinnedBuf<uint32_t> h_btile0;
  DevBuf<Key> d_bout;
  PinnedBuf<Key> h_bout;
  DevBuf<Key> d_bpart;
  // wide route
  DevBuf<Key> d_part;
  DevBuf<Segment> d_seg;
  PinnedBuf<Segment> h_seg;
  DevBuf<BatchSeg> d_gseg;
  PinnedBuf<BatchSeg> h_gseg;
  DevBuf<WideRange> d_wrange;
  PinnedBuf<WideRange> h_wrange;
  DevBuf<uint32_t> d_wrange0;
  PinnedBuf<uint32_t> h_wrange0;
  DevBuf<Key> d_wout;
  PinnedBuf<Key> h_wout;
  hipEvent_t done = nullptr;  // recorded after the ticket's last copy back (created on first use)
};

// Move-only (its buffers are): fine in std::vector<Dev> and for d = Dev().
struct Dev {
  int ordinal = -1;
  hipStream_t stream = nullptr;
  DevBuf<Key> d_part;           // one partial per tile of a scan
  DevBuf<Key> d_res;            // 1 Key
  DevBuf<Key> d_gather;         // ndev Keys (multi-device)
  PinnedBuf<Key> h_res;         // ndev Keys
  DevBuf<Segment> d_seg;        // segment tables, kMaxSegs per launch slot
  PinnedBuf<Segment> h_seg;     // staging for the tables
  ncclComm_t comm = nullptr;
  hipModule_t mod = nullptr;    // embedded code object, loaded on this device
  hipFunction_t f_scan = nullptr, f_reduce = nullptr, f_pairs = nullptr, f_small = nullptr, f_kwtable = nullptr;
  DevBuf<Key> d_small_part;     // kSmallMaxBlocks partials of k_scan_small
  DevBuf<uint32_t> d_ticket;    // k_scan_small's last-workgroup counter (0 between scans)
  DevBuf<uint32_t> d_scan_ticket;  // k_scan's work queue: [tiles handed out, workgroups done] (0 between launches)
  uint32_t scan_grid = 0;       // k_scan workgroups the device holds at once (occupancy x CUs)
  bool small_used = false;      // this scan ran k_scan_small (result already in h_res[0])
  // p1hip_scan_batch: its own code object and buffers (grown on demand, kept
  // across calls; no p1hip_scan touches them)
  hipModule_t bmod = nullptr;
  hipFunction_t f_bscan = nullptr, f_breduce = nullptr, f_wreduce = nullptr;
  DevBuf<BatchSeg> d_bseg;      // segment table of one launch pair
  PinnedBuf<BatchSeg> h_bseg;   // staging
  DevBuf<uint32_t> d_btile0;    // first tile of each request (+ end)
  PinnedBuf<uint32_t> h_btile0; // staging
  DevBuf<Key> d_bout;           // one Key per request
  PinnedBuf<Key> h_bout;
  DevBuf<Key> d_bpart;          // one partial per tile
  // p1hip_scan_batch_wide: its range table (the rest it shares: d_part, d_seg
  // and the ticket with p1hip_scan, d_bseg, d_btile0 and d_bout with the batch)
  DevBuf<WideRange> d_wrange;
  PinnedBuf<WideRange> h_wrange;
  // p1hip_scan_below: its own code object and buffers (the table and the
  // marks of one k_below_mark launch; its sparse slices run in p1hip_scan's)
  hipModule_t lmod = nullptr;
  hipFunction_t f_mark = nullptr;
  DevBuf<BatchSeg> d_mseg;
  PinnedBuf<BatchSeg> h_mseg;
  DevBuf<uint64_t> d_marks;     // kBelowWordsPerTile words per tile
  PinnedBuf<uint64_t> h_marks;
  // p1hip_scan_below_batch: its own code object and buffers.  The tables of
  // every launch pair of a round lie at their own offsets; the marks are one
  // launch pair's (the pairs of a device run in stream order); d_qout holds,
  // per launch pair, its requests' counts and then their hit indices, and is
  // copied back once per round.
  hipModule_t qmod = nullptr;
  hipFunction_t f_qmark = nullptr, f_qcollect = nullptr;
  DevBuf<BatchSeg> d_qseg;
  PinnedBuf<BatchSeg> h_qseg;
  DevBuf<uint64_t> d_qtarget;
  PinnedBuf<uint64_t> h_qtarget;
  DevBuf<uint32_t> d_qtab;      // per launch pair: req_tile0 (nreq + 1), req_hit0 (nreq + 1)
  PinnedBuf<uint32_t> h_qtab;
  DevBuf<uint64_t> d_qmarks;    // kBelowWordsPerTile words per tile
  DevBuf<uint32_t> d_qout;
  PinnedBuf<uint32_t> h_qout;
  // p1hip_scan_below_batch_wide: its own code object and buffers (phase A
  // shares d_part, d_seg and the ticket with p1hip_scan, d_bseg with the batch
  // and d_wrange with the wide call, as the wide call does).  d_ftab holds
  // req_range0 (nreq + 1) and req_slot0 (nreq + 1); d_fcand the requests'
  // counts and then their candidate slots; h_fpart the candidates' partials;
  // the rest is phase B's mark launch.
  hipModule_t fmod = nullptr;
  hipFunction_t f_wfilter = nullptr;
  DevBuf<uint32_t> d_ftab;
  PinnedBuf<uint32_t> h_ftab;
  DevBuf<uint64_t> d_ftarget;
  PinnedBuf<uint64_t> h_ftarget;
  DevBuf<uint32_t> d_fcand;
  PinnedBuf<uint32_t> h_fcand;
  PinnedBuf<Key> h_fpart;
  DevBuf<BatchSeg> d_fseg;
  PinnedBuf<BatchSeg> h_fseg;
  DevBuf<uint64_t> d_fmtarget;
  PinnedBuf<uint64_t> h_fmtarget;
  DevBuf<uint64_t> d_fmarks;
  PinnedBuf<uint64_t> h_fmarks;
  SlotDev slot[P1HIP_MAX_INFLIGHT];  // p1hip_batch_submit: one buffer set per ticket slot
  std::vector<hipEvent_t> evs;  // profiling event pool (pairs)
  // MODE 5 K+W tables on this device, least recently used first (built by
  // k_kwtable; keyed by the block-1 template and k)
  struct KwTab {
    uint32_t w[16];
    int k;
    uint32_t* dptr;
    uint64_t used_in;  // run_range call that last used it (never evicted during it)
  };
  std::vector<KwTab> kwtabs;
  uint64_t range_id = 0;        // run_range calls on this device
  ScanCounters ctr;             // per-scan accounting (run_small, run_range, run_share)
  uint64_t replans = 0;         // shares re-planned without MODE 5 (this scan)
  // since p1hip_reset_stats, for p1hip_get_device_stats
  p1hip_device_stats_t acc{};
};

// What p1hip_batch_wait needs of a submitted call (host memory only).
struct AsyncCall {
  size_t n = 0;
  std::vector<p1hip_result_t> res;  // empty ranges are already answered
  // where the coalesced results land: h_out[r] (pinned, the slot's) is request reqs[r]'s
  struct Part {
    const Key* h_out;
    std::vector<size_t> reqs;
  };
  std::vector<Part> parts;
  std::vector<char> dev_used;  // per device: the ticket recorded its event there
  // individual-route requests, run by the wait (their messages are copies)
  struct Indiv {
    size_t idx;
    std::string msg;
    uint64_t lower, upper;
  };
  std::vector<Indiv> indiv;
  // what the synchronous call would add to the statistics
  bool has_b = false, has_w = false;
  p1hip_batch_stats_t badd{};
  p1hip_wide_stats_t wadd{};
  double submit_ms = 0.0;
};

struct Runtime {
  std::mutex mu;
  // p1hip_batch_submit / p1hip_batch_wait: the tickets, their calls, and the
  // waits blocked on events with `mu` released (shutdown_locked waits for them)
  AsyncSlotsT<P1HIP_MAX_INFLIGHT> slots;
  AsyncCall calls[P1HIP_MAX_INFLIGHT];
  std::condition_variable cv;
  int blockers = 0;
  p1hip_async_stats_t astats{};
  std::vector<Dev> devs;
  bool profiling = false;
  // the kAtInit knobs, as the open devices were opened with
  bool use_rccl = true;   // multi-device combine through ncclAllGather
  bool rccl_one = false;  // communicator even for one device
  uint64_t min_fast_threads = kMinFastThreads;
  bool split = true;
  bool tabulate = true;
  int fail_device = -1;
  p1hip_stats_t stats{};
  p1hip_batch_stats_t bstats{};
  p1hip_wide_stats_t wstats{};
  p1hip_below_stats_t lstats{};
  p1hip_below_batch_stats_t qstats{};
  p1hip_below_wide_stats_t fstats{};
};

// Never destroyed: the runtime state outlives every static destructor, so a
// p1hip_* call made from a consumer's own atexit handler or static
// destructor still finds a valid mutex and device list, and the library
// issues no HIP call during process teardown (device memory is released
// only by p1hip_shutdown; what a process leaves open, the driver reclaims
// at exit).  The host containers it holds are reachable to the end.
Runtime& rt() {
  static Runtime* r = new Runtime();
  return *r;
}

// ----------------------------------------------------------------------------
// Helpers
// ----------------------------------------------------------------------------
int device_count(int* count) {
  *count = 0;
  if (hipGetDeviceCount(count) != hipSuccess || *count <= 0)
    return fail(P1HIP_ERR_NO_DEVICE, "no HIP device visible");
  return P1HIP_OK;
}

// hipModuleLaunchKernel with the arguments as a pointer array
template <typename... Args>
hipError_t launch(hipFunction_t f, uint32_t blocks, uint32_t threads, hipStream_t st, Args... args) {
  void* params[] = {(void*)&args...};
  return hipModuleLaunchKernel(f, blocks, 1, 1, threads, 1, 1, 0, st, params, nullptr);
}

// Profiling: scan launches sit between event pairs from the device's pool.
// ev_record records event `nev` (growing the pool) and counts it; ev_sum
// waits for the last one and adds every pair's elapsed time to scan_ms.
int ev_record(Dev& d, size_t& nev) {
  if (d.evs.size() <= nev) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    d.evs.push_back(e);
  }
  HIPCHK(hipEventRecord(d.evs[nev], d.stream));
  ++nev;
  return P1HIP_OK;
}

int ev_sum(Dev& d, size_t nev) {
  if (!nev) return P1HIP_OK;
  HIPCHK(hipEventSynchronize(d.evs[nev - 1]));
  for (size_t i = 0; i + 1 < nev; i += 2) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, d.evs[i], d.evs[i + 1]));
    d.ctr.scan_ms += ms;
  }
  return P1HIP_OK;
}

Key finish_key(Key k) {
  if (k.h == ~0ull) k.n = 0;  // identity (MaxUint64, 0) of miner.go:56
  return k;
}

void add_counters(p1hip_stats_t& s, const ScanCounters& c) {
  s.fast_launches += c.fast_launches;
  s.fast_nonces += c.fast_nonces;
  s.fast_alg_ops += c.fast_ops;
  s.generic_launches += c.gen_launches;
  s.generic_nonces += c.gen_nonces;
  s.scan_launches += c.scan_launches;
  s.scan_nonces += c.scan_nonces;
  s.scan_alg_ops += c.scan_ops;
  s.scan_kernel_ms += c.scan_ms;
}

void add_counters(p1hip_device_stats_t& a, const ScanCounters& c) {
  a.scans++;
  a.scan_launches += c.scan_launches;
  a.scan_nonces += c.scan_nonces;
  a.scan_alg_ops += c.scan_ops;
  a.scan_kernel_ms += c.scan_ms;
}

// ----------------------------------------------------------------------------
// Devices: open, close
// ----------------------------------------------------------------------------
int dev_release(Dev& d) {
  if (d.ordinal < 0) return 0;
  (void)hipSetDevice(d.ordinal);
  if (d.stream) (void)hipStreamSynchronize(d.stream);
  for (hipEvent_t e : d.evs) (void)hipEventDestroy(e);
  for (SlotDev& sd : d.slot)
    if (sd.done) (void)hipEventDestroy(sd.done);
  for (Dev::KwTab& t : d.kwtabs) (void)hipFree(t.dptr);
  if (d.comm) ncclCommDestroy(d.comm);
  if (d.stream) (void)hipStreamDestroy(d.stream);
  if (d.mod) (void)hipModuleUnload(d.mod);
  if (d.bmod) (void)hipModuleUnload(d.bmod);
  if (d.lmod) (void)hipModuleUnload(d.lmod);
  if (d.qmod) (void)hipModuleUnload(d.qmod);
  if (d.fmod) (void)hipModuleUnload(d.fmod);
  d = Dev();  // every Buf frees itself here: this device is current, its work is done
  return 0;
}

// With R.mu held by the caller.  Outstanding tickets are cancelled; a
// p1hip_batch_wait blocked on a ticket's events (with R.mu released) is let
// out first -- the streams are drained, so its events complete -- because the
// events and buffers it looks at are destroyed below.  It finds its ticket
// stale when it takes the mutex again.
void shutdown_locked(Runtime& R) {
  R.slots.CancelAll();
  if (R.blockers > 0) {
    for (Dev& d : R.devs)
      if (d.stream) (void)hipStreamSynchronize(d.stream);
    std::unique_lock<std::mutex> lk(R.mu, std::adopt_lock);
    R.cv.wait(lk, [&] { return R.blockers == 0; });
    lk.release();  // still locked: the caller's guard owns it
    R.slots.CancelAll();  // tickets issued while the mutex was released
  }
  for (AsyncCall& c : R.calls) c = AsyncCall();
  for (Dev& d : R.devs) dev_release(d);
  R.devs.clear();
}

int init_devs(Runtime& R, const std::vector<int>& ords) {
  int count = 0;
  if (int rc = device_count(&count)) return rc;
  const int nd = (int)ords.size();
  std::vector<int> cus(ords.size());
  for (int i = 0; i < nd; ++i) {
    const int o = ords[i];
    if (o < 0 || o >= count) return fail(P1HIP_ERR_NO_DEVICE, "device ordinal out of range: " + std::to_string(o));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, o));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
      return fail(P1HIP_ERR_NO_DEVICE, std::string("device is not gfx950: ") + prop.gcnArchName);
    cus[i] = prop.multiProcessorCount;
  }
  R.devs.resize(ords.size());
  for (int i = 0; i < nd; ++i) {
    Dev& d = R.devs[i];
    d.ordinal = ords[i];
    HIPCHK(hipSetDevice(d.ordinal));
    HIPCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    HIPCHK(hipModuleLoadData(&d.mod, p1hip_kernels_co));
    HIPCHK(hipModuleGetFunction(&d.f_scan, d.mod, "k_scan"));
    HIPCHK(hipModuleGetFunction(&d.f_reduce, d.mod, "k_reduce"));
    HIPCHK(hipModuleGetFunction(&d.f_pairs, d.mod, "k_pairs"));
    HIPCHK(hipModuleGetFunction(&d.f_small, d.mod, "k_scan_small"));
    HIPCHK(hipModuleGetFunction(&d.f_kwtable, d.mod, "k_kwtable"));
    HIPCHK(hipModuleLoadData(&d.bmod, p1hip_batch_co));
    HIPCHK(hipModuleGetFunction(&d.f_bscan, d.bmod, "k_batch_scan"));
    HIPCHK(hipModuleGetFunction(&d.f_breduce, d.bmod, "k_batch_reduce"));
    HIPCHK(hipModuleGetFunction(&d.f_wreduce, d.bmod, "k_wide_reduce"));
    HIPCHK(hipModuleLoadData(&d.lmod, p1hip_below_co));
    HIPCHK(hipModuleGetFunction(&d.f_mark, d.lmod, "k_below_mark"));
    HIPCHK(hipModuleLoadData(&d.qmod, p1hip_belowb_co));
    HIPCHK(hipModuleGetFunction(&d.f_qmark, d.qmod, "k_belowb_mark"));
    HIPCHK(hipModuleGetFunction(&d.f_qcollect, d.qmod, "k_belowb_collect"));
    HIPCHK(hipModuleLoadData(&d.fmod, p1hip_beloww_co));
    HIPCHK(hipModuleGetFunction(&d.f_wfilter, d.fmod, "k_beloww_filter"));
    // fixed-size buffers: floor = need, so exactly that many elements
    HIPCHK(d.d_small_part.reserve(kSmallMaxBlocks, kSmallMaxBlocks));
    HIPCHK(d.d_ticket.reserve(1, 1));
    HIPCHK(d.d_scan_ticket.reserve(2, 2));
    // on the library's own stream: a null-stream call would give every
    // process a second hardware queue (8 miner processes share one GPU)
    HIPCHK(hipMemsetAsync(d.d_ticket.p, 0, sizeof(uint32_t), d.stream));
    HIPCHK(hipMemsetAsync(d.d_scan_ticket.p, 0, 2 * sizeof(uint32_t), d.stream));
    // k_scan's grid: every workgroup slot of the device once (the work queue
    // hands the tiles out; p1hip_kernels.hip k_scan)
    int per_cu = 0;
    HIPCHK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, d.f_scan, kBlock, 0));
    if (per_cu < 1 || cus[i] < 1)
      return fail(P1HIP_ERR_HIP, "k_scan occupancy: " + std::to_string(per_cu) + " blocks per CU");
    d.scan_grid = (uint32_t)per_cu * (uint32_t)cus[i];
    HIPCHK(hipStreamSynchronize(d.stream));
    HIPCHK(d.d_res.reserve(1, 1));
    HIPCHK(d.d_gather.reserve((size_t)nd, (size_t)nd));
    HIPCHK(d.h_res.reserve((size_t)nd, (size_t)nd));
  }
  R.use_rccl = !knob(kNoRcclKnob);
  R.rccl_one = knob(kForceRcclKnob) && R.use_rccl;
  R.min_fast_threads = knob(kMinFastThreadsKnob);
  R.split = !knob(kNoSplitKnob);
  R.tabulate = !knob(kNoTableKnob);
  R.fail_device = (int)(int64_t)knob(kTestFailDeviceKnob);
  if ((nd > 1 || R.rccl_one) && R.use_rccl) {
    std::vector<ncclComm_t> comms(nd);
    NCCLCHK(ncclCommInitAll(comms.data(), nd, ords.data()));
    for (int i = 0; i < nd; ++i) R.devs[i].comm = comms[i];
  }
  return P1HIP_OK;
}

int init_locked(Runtime& R, const std::vector<int>& ords) {
  if (!R.devs.empty()) {
    bool same = R.devs.size() == ords.size();
    for (size_t i = 0; same && i < ords.size(); ++i) same = R.devs[i].ordinal == ords[i];
    if (same) return P1HIP_OK;
    shutdown_locked(R);
  }
  const int rc = init_devs(R, ords);
  if (rc != P1HIP_OK) {  // never leave a half-initialised device list behind
    const std::string keep = g_err;
    shutdown_locked(R);
    g_err = keep;
  }
  return rc;
}

int ensure_init(Runtime& R) {
  if (!R.devs.empty()) return P1HIP_OK;
  int count = 0;
  if (int rc = device_count(&count)) return rc;
  std::vector<int> ords;
  for (int i = 0; i < count; ++i) ords.push_back(i);
  return init_locked(R, ords);
}

// ----------------------------------------------------------------------------
// p1hip_scan
// ----------------------------------------------------------------------------
// The per-tile witness of p1hip_scan_tiles (test hook): run_small / run_range
// given one fill the scan's partials with P1HIP_TILE_POISON bytes before the
// first launch, and after the last they wait for the stream and copy the raw
// partials and the result back, next to the tile map of the plan they ran.
// The product path passes none: nothing is poisoned or copied there.
// p1hip_scan_below's sparse slices take the same map and partials as their
// filter: run_range without the poison (every partial of the scan is written)
// and without the collect, which follows once every device is enqueued.
struct TileDump {
  std::vector<TileInfo> map;
  std::vector<Key> part;
  Key res;
};

int dump_poison(Dev& d, Key* part, size_t n) {
  HIPCHK(hipMemsetAsync(part, P1HIP_TILE_POISON, n * sizeof(Key), d.stream));
  return P1HIP_OK;
}

int dump_collect(Dev& d, const Key* part, TileDump& dump) {
  dump.part.resize(dump.map.size());
  HIPCHK(hipMemcpyAsync(dump.part.data(), part, dump.part.size() * sizeof(Key), hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipMemcpyAsync(&dump.res, d.d_res.p, sizeof(Key), hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  return P1HIP_OK;
}

// Small share [lo, hi] (at most kSmallMaxNonces nonces): one k_scan_small
// launch; the Key lands in d.d_res and, when `to_host`, in d.h_res[0].
int run_small(Dev& d, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, bool to_host, bool profiling,
              TileDump* dump = nullptr) {
  HIPCHK(hipSetDevice(d.ordinal));
  d.ctr = {};
  Plan plan;
  std::string err = make_plan(msg, len, lo, hi, plan, false);
  if (!err.empty()) return fail(P1HIP_ERR_ARGS, "planner: " + err);
  SmallArgs a;
  err = fill_small(plan, a, d.ctr);
  if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
  a.part = d.d_small_part.p;
  a.ticket = d.d_ticket.p;
  a.out_dev = d.d_res.p;
  a.out_host = to_host ? d.h_res.p : nullptr;
  int rc;
  if (dump) {
    dump->map = tile_map_small(plan);
    if ((rc = dump_poison(d, a.part, a.nblocks))) return rc;
  }
  size_t nev = 0;
  if (profiling && (rc = ev_record(d, nev))) return rc;
  HIPCHK(launch(d.f_small, a.nblocks, kBlock, d.stream, a));
  if (profiling && (rc = ev_record(d, nev))) return rc;
  if ((rc = ev_sum(d, nev))) return rc;
  return dump ? dump_collect(d, a.part, *dump) : P1HIP_OK;
}

// Device copy of a MODE 5 launch's K+W table (cached, least recently used
// evicted: the same layout in later scans reuses it; scans are synchronous,
// so an evicted table is idle).
// kNoTable: the table cannot be had (larger than the cap, or the device is
// out of memory); the caller re-plans the share without MODE 5.
constexpr int kNoTable = 1;

int kwtable_for(Dev& d, const Launch& L, uint64_t* dptr) {
  for (size_t i = 0; i < d.kwtabs.size(); ++i) {
    Dev::KwTab t = d.kwtabs[i];
    if (t.k == L.tabk && memcmp(t.w, L.tabw, sizeof t.w) == 0) {
      t.used_in = d.range_id;
      // least recently used first: a scan touches at most 7 tables (one per
      // MODE 5 decade), so it never evicts one it is about to launch with
      d.kwtabs.erase(d.kwtabs.begin() + (long)i);
      d.kwtabs.push_back(t);
      *dptr = (uint64_t)(uintptr_t)t.dptr;
      return P1HIP_OK;
    }
  }
  const size_t need = (size_t)pow10u(L.tabk) * 64u * sizeof(uint32_t);
  const size_t cap = (size_t)knob(kKwtabMaxBytesKnob);
  if (need > cap) return kNoTable;
  for (;;) {
    size_t held = 0;
    for (const Dev::KwTab& t : d.kwtabs) held += (size_t)pow10u(t.k) * 64u * sizeof(uint32_t);
    if (d.kwtabs.empty() || (d.kwtabs.size() < kMaxKwTabs && held + need <= cap)) break;
    // evict the least recently used table this share has not referenced yet
    size_t v = 0;
    while (v < d.kwtabs.size() && d.kwtabs[v].used_in == d.range_id) ++v;
    if (v == d.kwtabs.size()) return kNoTable;  // everything held is in use by this share
    HIPCHK(hipFree(d.kwtabs[v].dptr));
    d.kwtabs.erase(d.kwtabs.begin() + (long)v);
  }
  // built on the device by k_kwtable, on the scan's stream (so the k_scan
  // launch that reads it is ordered after it): no host work, no upload
  Dev::KwTab t;
  memcpy(t.w, L.tabw, sizeof t.w);
  t.k = L.tabk;
  t.dptr = nullptr;
  t.used_in = d.range_id;
  const uint32_t rows = (uint32_t)pow10u(L.tabk);
  const hipError_t me = hipMalloc(&t.dptr, (size_t)rows * 64u * sizeof(uint32_t));
  if (me == hipErrorOutOfMemory) {
    (void)hipGetLastError();  // not sticky: clear it and scan without the table
    return kNoTable;
  }
  HIPCHK(me);
  KwTableArgs a;
  memset(&a, 0, sizeof a);
  memcpy(a.tabw, L.tabw, sizeof a.tabw);
  a.k = (uint32_t)L.tabk;
  a.qv = (uint32_t)(L.Y.q - 64);
  a.rows = rows;
  a.out = t.dptr;
  const hipError_t e = launch(d.f_kwtable, (rows + kBlock - 1) / kBlock, kBlock, d.stream, a);
  if (e != hipSuccess) {  // never cache a table that was not built
    (void)hipFree(t.dptr);
    return fail(P1HIP_ERR_HIP, std::string("k_kwtable launch: ") + hipGetErrorString(e));
  }
  d.kwtabs.push_back(t);
  *dptr = (uint64_t)(uintptr_t)t.dptr;
  return P1HIP_OK;
}

// k_scan's grid for a launch of `tiles` tiles: the device's workgroup slots,
// or P1HIP_SCAN_GRID
uint32_t scan_grid_for(const Dev& d, uint32_t tiles) {
  const uint64_t g = knob(kScanGridKnob);
  return std::min(tiles, g > 0 ? (uint32_t)g : d.scan_grid);
}

// Run one device's share [lo, hi] (lo <= hi) and leave its Key in d.d_res.
// With a `dump`: its map is filled in; `poison` fills the partials first and
// `collect` ends with dump_collect (else the caller collects).
int run_range(Dev& d, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, bool profiling,
              uint64_t min_fast_threads, bool split, bool tabulate, TileDump* dump = nullptr, bool poison = true,
              bool collect = true) {
  HIPCHK(hipSetDevice(d.ordinal));
  d.range_id++;  // tables referenced from here on are pinned until the next call
  d.ctr = {};
  Plan plan;
  // plan -> every MODE 5 table -> launches: a table that cannot be had makes
  // the share re-plan without MODE 5 here, before any k_scan of it (or any
  // segment-table copy) is enqueued, so nothing is scanned twice and no
  // buffer is reallocated behind queued work.  Tables already built stay
  // cached (their k_kwtable launches are complete work, not scan work).
  std::vector<uint64_t> tabptr;
  for (;;) {
    std::string err = make_plan(msg, len, lo, hi, plan, true, min_fast_threads, split, tabulate);
    if (!err.empty()) return fail(P1HIP_ERR_ARGS, "planner: " + err);
    tabptr.assign(plan.launches.size(), 0);
    bool replan = false;
    for (size_t i = 0; i < plan.launches.size() && !replan; ++i) {
      const Launch& L = plan.launches[i];
      if (!L.fast || (L.mode != 5 && L.mode != 7)) continue;
      const int rt = kwtable_for(d, L, &tabptr[i]);
      if (rt == kNoTable) replan = true;
      else if (rt != P1HIP_OK) return rt;
    }
    if (!replan) break;
    tabulate = false;  // the re-plan has no MODE 5 launch, so this loop ends
    d.replans++;
    plan = Plan();
  }
  const ScanPack P = pack_scan(plan, knob(kMaxLaunchBlocksKnob));
  HIPCHK(d.d_part.reserve(P.total_blocks, 1));
  HIPCHK(d.d_seg.reserve(P.batches.size() * kMaxSegs, 4 * kMaxSegs));
  HIPCHK(d.h_seg.reserve(P.batches.size() * kMaxSegs, 4 * kMaxSegs));
  int rc;
  if (dump) {
    dump->map = tile_map(plan, P);
    if (poison && (rc = dump_poison(d, d.d_part.p, P.total_blocks))) return rc;
  }
  size_t nev = 0;
  uint32_t part_off = 0;
  for (size_t bi = 0; bi < P.batches.size(); ++bi) {
    const ScanBatch& B = P.batches[bi];
    Segment* hs = d.h_seg.p + bi * kMaxSegs;
    Segment* ds = d.d_seg.p + bi * kMaxSegs;
    const std::string err = fill_segments(plan, P, B, tabptr.data(), hs, d.ctr);
    if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
    HIPCHK(hipMemcpyAsync(ds, hs, B.count * sizeof(Segment), hipMemcpyHostToDevice, d.stream));
    if (profiling && (rc = ev_record(d, nev))) return rc;
#ifdef P1_STATIC_GRID
    HIPCHK(launch(d.f_scan, B.blocks, kBlock, d.stream, (const Segment*)ds, (uint32_t)B.count,
                  (Key*)(d.d_part.p + part_off)));
#else
    // B.blocks tiles through a work queue on min(tiles, slots) workgroups
    HIPCHK(launch(d.f_scan, scan_grid_for(d, B.blocks), kBlock, d.stream, (const Segment*)ds,
                  (uint32_t)B.count, (Key*)(d.d_part.p + part_off), (uint32_t)B.blocks, d.d_scan_ticket.p));
#endif
    if (profiling && (rc = ev_record(d, nev))) return rc;
    part_off += B.blocks;
  }
  HIPCHK(launch(d.f_reduce, 1, kReduceThreads, d.stream, (const Key*)d.d_part.p, P.total_blocks, d.d_res.p));
  if ((rc = ev_sum(d, nev))) return rc;
  return dump && collect ? dump_collect(d, d.d_part.p, *dump) : P1HIP_OK;
}

// A device's share, in pieces of at most kMaxScanSpan nonces: the plan of a
// share is O(its size / 2^26 hi values), so a share as large as the whole
// u64 range (which the Go loop never finishes either) would need ~10^8
// pieces.  Each piece is a full run_range; the keys are combined on the host
// and the result written back to d.d_res.  Shares up to 2^40 nonces (about
// 30 s of one GPU) are a single piece, with no extra copy.
int run_share(Dev& d, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, const Runtime& R) {
  const uint64_t span = knob(kMaxScanSpanKnob);
  if (hi - lo < span)
    return run_range(d, msg, len, lo, hi, R.profiling, R.min_fast_threads, R.split, R.tabulate);
  Key best = {~0ull, ~0ull};
  ScanCounters sum;
  for (uint64_t a = lo;;) {
    const uint64_t b = hi - a < span ? hi : a + (span - 1);
    int r = run_range(d, msg, len, a, b, R.profiling, R.min_fast_threads, R.split, R.tabulate);
    if (r != P1HIP_OK) return r;
    Key k;
    HIPCHK(hipMemcpyAsync(&k, d.d_res.p, sizeof(Key), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    if (key_lt(k, best)) best = k;
    sum += d.ctr;
    if (b == hi) break;
    a = b + 1;
  }
  d.ctr = sum;
  HIPCHK(hipMemcpyAsync(d.d_res.p, &best, sizeof(Key), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));  // `best` lives on this stack frame
  return P1HIP_OK;
}

// One scan with R.mu held by the caller (p1hip_scan; p1hip_scan_batch for the
// requests it runs individually).
int scan_held(Runtime& R, const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
              uint64_t* out_nonce) {
  const auto t0 = std::chrono::steady_clock::now();
  int rc = ensure_init(R);
  if (rc) return rc;
  Key res = {~0ull, 0};
  if (lower <= upper) {
    const size_t nd = R.devs.size();
    // contiguous shards of near-equal predicted cost (planner.hpp plan_shards)
    std::vector<uint64_t> slo(nd), shi(nd);
    std::vector<char> active(nd, 0);
    plan_shards(msg, msg_len, lower, upper, (int)nd, slo.data(), shi.data());
    for (size_t i = 0; i < nd; ++i) active[i] = slo[i] <= shi[i];
    // Phase 1: every device scans its shard and synchronises its stream.
    // Phase 2 (the collective) starts only when every device succeeded, so a
    // failing device can never leave its peers blocked inside ncclAllGather.
    std::vector<int> rcs(nd, 0);
    std::vector<std::string> errs(nd);
    auto run_threads = [&](auto&& fn) {
      if (nd == 1) {
        fn(0);
      } else {
        // every thread is created before any of them runs `fn`: if one cannot
        // start, none enters the scan or the collective (a peer blocked in
        // ncclAllGather waiting for a thread that never started would hang)
        std::atomic<int> go{0};  // 0 wait, 1 run, -1 abort
        std::vector<std::thread> th;
        try {
          for (size_t i = 0; i < nd; ++i)
            th.emplace_back([&, i]() {
              while (go.load(std::memory_order_acquire) == 0) std::this_thread::yield();
              if (go.load(std::memory_order_acquire) == 1) fn(i);
            });
        } catch (...) {
          go.store(-1, std::memory_order_release);
          for (auto& t : th) t.join();
          throw;
        }
        go.store(1, std::memory_order_release);
        for (auto& t : th) t.join();
      }
    };
    // One phase on every device: body(i, d) is device i's work and returns
    // its rc.  A host exception inside a device thread would end the process
    // (std::terminate): it becomes this device's rc instead, with the message
    // if building it does not throw as well.  The phase's wall time is added
    // to the device's `ms`.
    auto run_phase = [&](double p1hip_device_stats_t::*ms, auto&& body) {
      run_threads([&](size_t i) {
        Dev& d = R.devs[i];
        const auto p0 = std::chrono::steady_clock::now();
        int r;
        try {
          r = body(i, d);
        } catch (const std::exception& ex) {
          try {
            r = fail(P1HIP_ERR_HIP, std::string("host: ") + ex.what());
          } catch (...) {
            r = P1HIP_ERR_HIP;
          }
        } catch (...) {
          r = P1HIP_ERR_HIP;
        }
        d.acc.*ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
        rcs[i] = r;
        if (r) {
          try {
            errs[i] = g_err;
          } catch (...) {  // the copy allocates; rcs[i] already says what matters
          }
        }
      });
      for (size_t i = 0; i < nd; ++i)
        if (rcs[i]) return fail(rcs[i], "device " + std::to_string(R.devs[i].ordinal) + ": " + errs[i]);
      return (int)P1HIP_OK;
    };
    const bool coll = (nd > 1 || R.rccl_one) && R.use_rccl;
    const uint64_t small_max = knob(kSmallMaxNoncesKnob);
    rc = run_phase(&p1hip_device_stats_t::phase1_ms, [&](size_t i, Dev& d) -> int {
      // per-scan accounting starts empty on every device (an inactive shard
      // must not re-report its previous scan)
      d.ctr = {};
      d.replans = 0;
      d.small_used = false;
      d.acc.shard_first = slo[i];
      d.acc.shard_last = shi[i];
      d.acc.active = active[i];
      int r = P1HIP_OK;
      if ((int)i == R.fail_device) {
        r = fail(P1HIP_ERR_HIP, "injected failure (P1HIP_TEST_FAIL_DEVICE)");
      } else if (active[i] && shi[i] - slo[i] < small_max) {
        d.small_used = true;
        r = run_small(d, msg, msg_len, slo[i], shi[i], !coll && nd == 1, R.profiling);
      } else if (active[i]) {
        r = run_share(d, msg, msg_len, slo[i], shi[i], R);
      } else {
        // empty shard: contribute the identity key (all ones)
        if (hipSetDevice(d.ordinal) != hipSuccess) r = fail(P1HIP_ERR_HIP, "hipSetDevice");
        if (!r && hipMemsetAsync(d.d_res.p, 0xFF, sizeof(Key), d.stream) != hipSuccess)
          r = fail(P1HIP_ERR_HIP, "hipMemsetAsync(identity)");
      }
      if (!r && !coll && nd > 1) {  // host combine (P1HIP_NO_RCCL, tests)
        if (hipMemcpyAsync(R.devs[0].h_res.p + i, d.d_res.p, sizeof(Key), hipMemcpyDeviceToHost, d.stream) !=
            hipSuccess)
          r = fail(P1HIP_ERR_HIP, "hipMemcpyAsync(result)");
      } else if (!r && !coll && !(active[i] && d.small_used)) {  // the small kernel wrote h_res itself
        if (hipMemcpyAsync(d.h_res.p, d.d_res.p, sizeof(Key), hipMemcpyDeviceToHost, d.stream) != hipSuccess)
          r = fail(P1HIP_ERR_HIP, "hipMemcpyAsync(result)");
      }
      if (!r && hipStreamSynchronize(d.stream) != hipSuccess) r = fail(P1HIP_ERR_HIP, "hipStreamSynchronize");
      return r;
    });
    if (rc != P1HIP_OK) return rc;
    if (coll) {
      // Phase 2: all-gather the 16-byte partials (2 x u64 per device) over
      // RCCL; device 0 copies the gathered table to the host.  One group call
      // per device thread is not needed: each thread enqueues on its own
      // communicator and the collective completes when all have joined.
      rc = run_phase(&p1hip_device_stats_t::gather_ms, [&](size_t i, Dev& d) -> int {
        if (hipSetDevice(d.ordinal) != hipSuccess) return fail(P1HIP_ERR_HIP, "hipSetDevice");
        ncclResult_t nr = ncclAllGather(d.d_res.p, d.d_gather.p, 2, ncclUint64, d.comm, d.stream);
        if (nr != ncclSuccess) return fail(P1HIP_ERR_RCCL, std::string("ncclAllGather: ") + ncclGetErrorString(nr));
        if (i == 0 &&
            hipMemcpyAsync(d.h_res.p, d.d_gather.p, sizeof(Key) * nd, hipMemcpyDeviceToHost, d.stream) != hipSuccess)
          return fail(P1HIP_ERR_HIP, "hipMemcpyAsync(gathered)");
        if (hipStreamSynchronize(d.stream) != hipSuccess) return fail(P1HIP_ERR_HIP, "hipStreamSynchronize");
        return P1HIP_OK;
      });
      if (rc != P1HIP_OK) return rc;
    }
    Key b = {~0ull, ~0ull};
    for (size_t i = 0; i < nd; ++i) b = key_lt(R.devs[0].h_res.p[i], b) ? R.devs[0].h_res.p[i] : b;
    res = finish_key(b);
    for (Dev& d : R.devs) {
      add_counters(R.stats, d.ctr);
      add_counters(d.acc, d.ctr);
      if (d.small_used && d.ctr.scan_launches) R.stats.small_scans++;
      R.stats.table_replans += d.replans;
    }
  }
  R.stats.scans++;
  R.stats.scan_wall_ms +=
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out_hash = res.h;
  *out_nonce = res.n;
  return P1HIP_OK;
}

int scan_locked(const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
                uint64_t* out_nonce) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  return scan_held(R, msg, msg_len, lower, upper, out_hash, out_nonce);
}

// ----------------------------------------------------------------------------
// p1hip_scan_batch
// ----------------------------------------------------------------------------
int batch_check(const p1hip_request_t* reqs, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    if (!reqs[i].msg && reqs[i].msg_len > 0)
      return fail(P1HIP_ERR_ARGS, "request " + std::to_string(i) + ": msg == NULL with msg_len > 0");
    if (reqs[i].msg_len > P1HIP_MAX_MSG_LEN)
      return fail(P1HIP_ERR_ARGS, "request " + std::to_string(i) + ": msg_len exceeds P1HIP_MAX_MSG_LEN");
  }
  return P1HIP_OK;
}

std::vector<BatchReq> batch_reqs(const p1hip_request_t* reqs, size_t n) {
  std::vector<BatchReq> q(n);
  for (size_t i = 0; i < n; ++i) q[i] = {reqs[i].msg, reqs[i].msg_len, reqs[i].lower, reqs[i].upper};
  return q;
}

// Room on device d for a launch pair of `nseg` segments, `nreq` requests and
// `tiles` tiles.  Called only while the stream is idle (every round of
// scan_batch_locked ends with a synchronisation).
int batch_reserve(Dev& d, size_t nseg, size_t nreq, size_t tiles) {
  HIPCHK(d.d_bseg.reserve(nseg, 64));
  HIPCHK(d.h_bseg.reserve(nseg, 64));
  HIPCHK(d.d_btile0.reserve(nreq, 64, 1));
  HIPCHK(d.h_btile0.reserve(nreq, 64, 1));
  HIPCHK(d.d_bout.reserve(nreq, 64));
  HIPCHK(d.h_bout.reserve(nreq, 64));
  HIPCHK(d.d_bpart.reserve(tiles, 1024));
  return P1HIP_OK;
}

// The buffers one launch pair runs in: the Dev's own (the synchronous calls),
// or a place in a ticket slot's (p1hip_batch_submit).
struct BatchBufs {
  BatchSeg *d_seg, *h_seg;
  uint32_t *d_tile0, *h_tile0;
  Key *d_out, *h_out, *d_part;
};

// Enqueue launch pair L (tables T) on device d's stream: the tables, k_batch_scan,
// k_batch_reduce and the copy back.  No synchronisation.
int batch_enqueue(Dev& d, const BatchLaunch& L, const BatchTable& T, const BatchBufs& b) {
  const size_t nseg = T.segs.size(), nreq = L.reqs.size();
  memcpy(b.h_seg, T.segs.data(), nseg * sizeof(BatchSeg));
  memcpy(b.h_tile0, T.req_tile0.data(), (nreq + 1) * sizeof(uint32_t));
  HIPCHK(hipMemcpyAsync(b.d_seg, b.h_seg, nseg * sizeof(BatchSeg), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(b.d_tile0, b.h_tile0, (nreq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
  HIPCHK(launch(d.f_bscan, L.tiles, kBlock, d.stream, (const BatchSeg*)b.d_seg, (uint32_t)nseg, b.d_part));
  HIPCHK(launch(d.f_breduce, (uint32_t)nreq, kBlock, d.stream, (const Key*)b.d_part, (const uint32_t*)b.d_tile0,
                b.d_out));
  HIPCHK(hipMemcpyAsync(b.h_out, b.d_out, nreq * sizeof(Key), hipMemcpyDeviceToHost, d.stream));
  return P1HIP_OK;
}

// One p1hip_scan_batch with R.mu held by the caller (p1hip_scan_batch;
// p1hip_scan_batch_wide for its small requests).
int scan_batch_held(Runtime& R, const p1hip_request_t* reqs, size_t n, p1hip_result_t* out) {
  const auto t0 = std::chrono::steady_clock::now();
  int rc = ensure_init(R);
  if (rc) return rc;
  const std::vector<BatchReq> q = batch_reqs(reqs, n);
  const BatchLayout Y =
      batch_layout(q.data(), n, (int)R.devs.size(), knob(kBatchMaxNoncesKnob), knob(kBatchMaxTilesKnob));
  // results are gathered here and copied to `out` only when the whole call
  // has succeeded
  std::vector<p1hip_result_t> res(n, p1hip_result_t{~0ull, 0});
  // Coalesced requests, in rounds: round k enqueues launch pair k of every
  // device that has one (tables, k_batch_scan, k_batch_reduce, copy back, all
  // on the device's stream) and only then synchronises those streams: one
  // synchronisation per launch pair, and the devices run side by side.
  uint64_t tiles = 0, nonces = 0;
  auto run = [&]() -> int {
    BatchTable T;
    std::vector<const BatchLaunch*> round;
    for (int k = 0;; ++k) {
      round.clear();
      for (const BatchLaunch& L : Y.launches)
        if (L.launch == k) round.push_back(&L);
      if (round.empty()) break;
      for (const BatchLaunch* L : round) {
        Dev& d = R.devs[(size_t)L->device];
        std::string err = batch_build_table(q.data(), *L, T);
        if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
        const size_t nseg = T.segs.size(), nreq = L->reqs.size();
        HIPCHK(hipSetDevice(d.ordinal));
        if ((rc = batch_reserve(d, nseg, nreq, L->tiles)) != P1HIP_OK) return rc;
        const BatchBufs b = {d.d_bseg.p, d.h_bseg.p, d.d_btile0.p, d.h_btile0.p, d.d_bout.p, d.h_bout.p, d.d_bpart.p};
        if ((rc = batch_enqueue(d, *L, T, b)) != P1HIP_OK) return rc;
        tiles += L->tiles;
        nonces += T.nonces;
      }
      for (const BatchLaunch* L : round) {
        Dev& d = R.devs[(size_t)L->device];
        HIPCHK(hipStreamSynchronize(d.stream));
        for (size_t r = 0; r < L->reqs.size(); ++r) {
          const Key kq = finish_key(d.h_bout.p[r]);
          res[L->reqs[r]] = p1hip_result_t{kq.h, kq.n};
        }
      }
    }
    // Larger requests: one by one through the multi-device scan path.
    if (Y.individual)
      for (size_t i = 0; i < n; ++i)
        if (q[i].lower <= q[i].upper && Y.tiles[i] == 0) {
          rc = scan_held(R, q[i].msg, q[i].len, q[i].lower, q[i].upper, &res[i].hash, &res[i].nonce);
          if (rc) return fail(rc, "request " + std::to_string(i) + ": " + g_err);
        }
    return P1HIP_OK;
  };
  if ((rc = run()) != P1HIP_OK) {
    // leave no launch pair in flight behind a failed call: the next call
    // rewrites the pinned staging tables
    const std::string keep = g_err;
    for (Dev& d : R.devs) (void)hipStreamSynchronize(d.stream);
    g_err = keep;
    return rc;
  }
  for (size_t i = 0; i < n; ++i) out[i] = res[i];
  R.bstats.calls++;
  R.bstats.requests += n;
  R.bstats.coalesced += Y.coalesced;
  R.bstats.individual += Y.individual;
  R.bstats.empty += Y.empty;
  R.bstats.launches += Y.launches.size();
  R.bstats.tiles += tiles;
  R.bstats.nonces += nonces;
  R.bstats.wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return P1HIP_OK;
}

int scan_batch_locked(const p1hip_request_t* reqs, size_t n, p1hip_result_t* out) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  return scan_batch_held(R, reqs, n, out);
}

// ----------------------------------------------------------------------------
// p1hip_scan_batch_wide
// ----------------------------------------------------------------------------
// The layout of a wide call as the knobs in force give it (R.mu held: the
// split setting is the open devices', or the environment's before any init).
std::string wide_layout_held(const Runtime& R, const std::vector<BatchReq>& q, int ndev, WideLayout& Y) {
  const bool split = R.devs.empty() ? !knob(kNoSplitKnob) : R.split;
  return wide_layout(q.data(), q.size(), ndev, knob(kBatchMaxNoncesKnob), knob(kWideMaxNoncesKnob),
                     (uint32_t)knob(kWideMaxSegsKnob), knob(kWideMinFastThreadsKnob), split, Y);
}

// Room on device d for its part of a wide call.  Called only while the stream
// is idle (every call ends with a synchronisation).
int wide_reserve(Dev& d, const WideDevice& D) {
  const size_t nreq = D.reqs.size();
  HIPCHK(d.d_part.reserve(D.total_tiles, 1));
  HIPCHK(d.d_seg.reserve(D.fast.size(), 4 * kMaxSegs));
  HIPCHK(d.h_seg.reserve(D.fast.size(), 4 * kMaxSegs));
  HIPCHK(d.d_bseg.reserve(D.gsegs.size(), 64));
  HIPCHK(d.h_bseg.reserve(D.gsegs.size(), 64));
  HIPCHK(d.d_wrange.reserve(D.ranges.size(), 64));
  HIPCHK(d.h_wrange.reserve(D.ranges.size(), 64));
  HIPCHK(d.d_btile0.reserve(nreq, 64, 1));
  HIPCHK(d.h_btile0.reserve(nreq, 64, 1));
  HIPCHK(d.d_bout.reserve(nreq, 64));
  HIPCHK(d.h_bout.reserve(nreq, 64));
  return P1HIP_OK;
}

// Enqueue device d's part of a wide call on its stream: the tables, one
// k_batch_scan for the generic pieces, the k_scan launches back to back (the
// ticket is zero between launches, as in a multi-launch p1hip_scan), the
// per-request fold and the copy back.  No synchronisation.
// `b`: the buffers it runs in, the Dev's own (wide_reserve; the synchronous
// call) or a ticket slot's (p1hip_batch_submit).  The work-queue ticket is the
// device's in both cases: launches on one stream run in order.
struct WideBufs {
  Key* d_part;
  Segment *d_seg, *h_seg;
  BatchSeg *d_gseg, *h_gseg;
  WideRange *d_range, *h_range;
  uint32_t *d_range0, *h_range0;
  Key *d_out, *h_out;
};

int wide_enqueue(Dev& d, const WideDevice& D, const WideBufs& b) {
  const size_t nreq = D.reqs.size();
  // segment tables of all k_scan launches, back to back (W.first is the launch's offset)
  for (const WideLaunch& W : D.launches) {
    const std::string err = wide_fill_launch(D, W, b.h_seg + W.first);
    if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
  }
  if (!D.fast.empty())
    HIPCHK(hipMemcpyAsync(b.d_seg, b.h_seg, D.fast.size() * sizeof(Segment), hipMemcpyHostToDevice, d.stream));
  memcpy(b.h_range, D.ranges.data(), D.ranges.size() * sizeof(WideRange));
  memcpy(b.h_range0, D.req_range0.data(), (nreq + 1) * sizeof(uint32_t));
  HIPCHK(hipMemcpyAsync(b.d_range, b.h_range, D.ranges.size() * sizeof(WideRange), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(b.d_range0, b.h_range0, (nreq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
  if (D.gen_tiles) {
    memcpy(b.h_gseg, D.gsegs.data(), D.gsegs.size() * sizeof(BatchSeg));
    HIPCHK(hipMemcpyAsync(b.d_gseg, b.h_gseg, D.gsegs.size() * sizeof(BatchSeg), hipMemcpyHostToDevice, d.stream));
    HIPCHK(launch(d.f_bscan, D.gen_tiles, kBlock, d.stream, (const BatchSeg*)b.d_gseg, (uint32_t)D.gsegs.size(),
                  (Key*)(b.d_part + D.gen_tile0)));
  }
  for (const WideLaunch& W : D.launches) {
#ifdef P1_STATIC_GRID
    HIPCHK(launch(d.f_scan, W.tiles, kBlock, d.stream, (const Segment*)(b.d_seg + W.first), (uint32_t)W.count,
                  (Key*)(b.d_part + W.tile0)));
#else
    HIPCHK(launch(d.f_scan, scan_grid_for(d, W.tiles), kBlock, d.stream, (const Segment*)(b.d_seg + W.first),
                  (uint32_t)W.count, (Key*)(b.d_part + W.tile0), (uint32_t)W.tiles, d.d_scan_ticket.p));
#endif
  }
  HIPCHK(launch(d.f_wreduce, (uint32_t)nreq, kBlock, d.stream, (const Key*)b.d_part, (const WideRange*)b.d_range,
                (const uint32_t*)b.d_range0, b.d_out));
  HIPCHK(hipMemcpyAsync(b.h_out, b.d_out, nreq * sizeof(Key), hipMemcpyDeviceToHost, d.stream));
  return P1HIP_OK;
}

// The synchronous call's: in the Dev's own buffers.
int wide_enqueue(Dev& d, const WideDevice& D) {
  HIPCHK(hipSetDevice(d.ordinal));
  int rc = wide_reserve(d, D);
  if (rc) return rc;
  const WideBufs b = {d.d_part.p,   d.d_seg.p,    d.h_seg.p,    d.d_bseg.p, d.h_bseg.p, d.d_wrange.p,
                      d.h_wrange.p, d.d_btile0.p, d.h_btile0.p, d.d_bout.p, d.h_bout.p};
  return wide_enqueue(d, D, b);
}

int scan_batch_wide_locked(const p1hip_request_t* reqs, size_t n, p1hip_result_t* out) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  const auto t0 = std::chrono::steady_clock::now();
  int rc = ensure_init(R);
  if (rc) return rc;
  const std::vector<BatchReq> q = batch_reqs(reqs, n);
  WideLayout Y;
  const std::string lerr = wide_layout_held(R, q, (int)R.devs.size(), Y);
  if (!lerr.empty()) return fail(P1HIP_ERR_ARGS, lerr);
  // results are gathered here and copied to `out` only when the whole call has succeeded
  std::vector<p1hip_result_t> res(n, p1hip_result_t{~0ull, 0});
  // Small requests: p1hip_scan_batch's own path, as one batch.
  if (Y.small) {
    std::vector<p1hip_request_t> sq;
    std::vector<size_t> idx;
    for (size_t i = 0; i < n; ++i)
      if (Y.route[i] == kWideRouteSmall) {
        sq.push_back(reqs[i]);
        idx.push_back(i);
      }
    std::vector<p1hip_result_t> so(sq.size());
    if ((rc = scan_batch_held(R, sq.data(), sq.size(), so.data())) != P1HIP_OK) return rc;
    for (size_t j = 0; j < idx.size(); ++j) res[idx[j]] = so[j];
  }
  // Wide requests: every device's launches are enqueued before any stream is
  // synchronised, so the devices run side by side.
  p1hip_wide_stats_t add{};
  auto run = [&]() -> int {
    for (size_t dv = 0; dv < Y.devs.size(); ++dv) {
      const WideDevice& D = Y.devs[dv];
      if (D.reqs.empty()) continue;
      if ((rc = wide_enqueue(R.devs[dv], D)) != P1HIP_OK) return rc;
      add.scan_launches += D.launches.size();
      add.scan_segments += D.fast.size();
      add.generic_launches += D.gen_tiles ? 1 : 0;
      add.generic_segments += D.gsegs.size();
      add.tiles += D.total_tiles;
      add.nonces += D.nonces;
    }
    for (size_t dv = 0; dv < Y.devs.size(); ++dv) {
      const WideDevice& D = Y.devs[dv];
      if (D.reqs.empty()) continue;
      Dev& d = R.devs[dv];
      HIPCHK(hipStreamSynchronize(d.stream));
      for (size_t r = 0; r < D.reqs.size(); ++r) {
        const Key kq = finish_key(d.h_bout.p[r]);
        res[D.reqs[r]] = p1hip_result_t{kq.h, kq.n};
      }
    }
    // Larger requests: one by one through the multi-device scan path.
    for (size_t i = 0; i < n; ++i)
      if (Y.route[i] == kWideRouteIndividual) {
        rc = scan_held(R, q[i].msg, q[i].len, q[i].lower, q[i].upper, &res[i].hash, &res[i].nonce);
        if (rc) return fail(rc, "request " + std::to_string(i) + ": " + g_err);
      }
    return P1HIP_OK;
  };
  if ((rc = run()) != P1HIP_OK) {
    // leave nothing in flight behind a failed call: the next call rewrites the pinned staging tables
    const std::string keep = g_err;
    for (Dev& d : R.devs) (void)hipStreamSynchronize(d.stream);
    g_err = keep;
    return rc;
  }
  for (size_t i = 0; i < n; ++i) out[i] = res[i];
  p1hip_wide_stats_t& S = R.wstats;
  S.calls++;
  S.requests += n;
  S.empty += Y.empty;
  S.small += Y.small;
  S.wide += Y.wide;
  S.individual += Y.individual;
  S.scan_launches += add.scan_launches;
  S.scan_segments += add.scan_segments;
  S.generic_launches += add.generic_launches;
  S.generic_segments += add.generic_segments;
  S.tiles += add.tiles;
  S.nonces += add.nonces;
  S.wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return P1HIP_OK;
}

// ----------------------------------------------------------------------------
// p1hip_batch_submit / p1hip_batch_wait
// ----------------------------------------------------------------------------
// Lay the call out as the synchronous call would, enqueue its empty, small and
// wide routes in slot `s`'s buffers and record one event per device used.
// R.mu held; the slot is the caller's.  No synchronisation.
int submit_enqueue(Runtime& R, int s, AsyncCall& C, const p1hip_request_t* reqs, size_t n, bool wide) {
  const std::vector<BatchReq> q = batch_reqs(reqs, n);
  const size_t nd = R.devs.size();
  C.n = n;
  C.res.assign(n, p1hip_result_t{~0ull, 0});
  C.dev_used.assign(nd, 0);
  auto individual = [&](size_t i) {
    C.indiv.push_back({i, std::string((const char*)q[i].msg, q[i].len), q[i].lower, q[i].upper});
  };
  // The requests of the small route: all of them for p1hip_scan_batch; for
  // the wide call its route-1 requests, as one batch (scan_batch_wide_locked).
  std::vector<BatchReq> sq;
  std::vector<size_t> sidx;
  WideLayout W;
  if (wide) {
    const std::string lerr = wide_layout_held(R, q, (int)nd, W);
    if (!lerr.empty()) return fail(P1HIP_ERR_ARGS, lerr);
    for (size_t i = 0; i < n; ++i) {
      if (W.route[i] == kWideRouteSmall) {
        sq.push_back(q[i]);
        sidx.push_back(i);
      } else if (W.route[i] == kWideRouteIndividual) {
        individual(i);
      }
    }
    C.has_w = true;
    C.wadd.requests = n;
    C.wadd.empty = W.empty;
    C.wadd.small = W.small;
    C.wadd.wide = W.wide;
    C.wadd.individual = W.individual;
  } else {
    sq = q;
    for (size_t i = 0; i < n; ++i) sidx.push_back(i);
  }
  int rc;
  if (!wide || W.small) {
    const BatchLayout Y =
        batch_layout(sq.data(), sq.size(), (int)nd, knob(kBatchMaxNoncesKnob), knob(kBatchMaxTilesKnob));
    for (size_t j = 0; j < sq.size(); ++j)
      if (sq[j].lower <= sq[j].upper && Y.tiles[j] == 0) individual(sidx[j]);
    C.has_b = true;
    C.badd.requests = sq.size();
    C.badd.coalesced = Y.coalesced;
    C.badd.individual = Y.individual;
    C.badd.empty = Y.empty;
    C.badd.launches = Y.launches.size();
    // every launch pair of a device gets a place of its own in the slot's
    // buffers (the synchronous call reuses one place and synchronises between
    // the pairs), so the tables are built first and the room reserved once
    std::vector<BatchTable> T(Y.launches.size());
    struct Need {
      size_t seg = 0, req = 0, tile0 = 0, tiles = 0;
    };
    std::vector<Need> need(nd);
    for (size_t li = 0; li < Y.launches.size(); ++li) {
      const BatchLaunch& L = Y.launches[li];
      const std::string err = batch_build_table(sq.data(), L, T[li]);
      if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
      Need& N = need[(size_t)L.device];
      N.seg += T[li].segs.size();
      N.req += L.reqs.size();
      N.tile0 += L.reqs.size() + 1;
      N.tiles += L.tiles;
      C.badd.tiles += L.tiles;
      C.badd.nonces += T[li].nonces;
    }
    for (size_t dv = 0; dv < nd; ++dv) {
      const Need& N = need[dv];
      if (!N.req) continue;
      Dev& d = R.devs[dv];
      SlotDev& sd = d.slot[s];
      HIPCHK(hipSetDevice(d.ordinal));
      HIPCHK(sd.d_bseg.reserve(N.seg, 64));
      HIPCHK(sd.h_bseg.reserve(N.seg, 64));
      HIPCHK(sd.d_btile0.reserve(N.tile0, 64));
      HIPCHK(sd.h_btile0.reserve(N.tile0, 64));
      HIPCHK(sd.d_bout.reserve(N.req, 64));
      HIPCHK(sd.h_bout.reserve(N.req, 64));
      HIPCHK(sd.d_bpart.reserve(N.tiles, 1024));
      Need at;
      for (size_t li = 0; li < Y.launches.size(); ++li) {
        const BatchLaunch& L = Y.launches[li];
        if ((size_t)L.device != dv) continue;
        const BatchBufs b = {sd.d_bseg.p + at.seg,     sd.h_bseg.p + at.seg, sd.d_btile0.p + at.tile0,
                             sd.h_btile0.p + at.tile0, sd.d_bout.p + at.req, sd.h_bout.p + at.req,
                             sd.d_bpart.p + at.tiles};
        if ((rc = batch_enqueue(d, L, T[li], b)) != P1HIP_OK) return rc;
        C.dev_used[dv] = 1;
        AsyncCall::Part P;
        P.h_out = b.h_out;
        for (size_t r : L.reqs) P.reqs.push_back(sidx[r]);
        C.parts.push_back(std::move(P));
        at.seg += T[li].segs.size();
        at.req += L.reqs.size();
        at.tile0 += L.reqs.size() + 1;
        at.tiles += L.tiles;
      }
    }
  }
  if (wide)
    for (size_t dv = 0; dv < W.devs.size(); ++dv) {
      const WideDevice& D = W.devs[dv];
      if (D.reqs.empty()) continue;
      Dev& d = R.devs[dv];
      SlotDev& sd = d.slot[s];
      const size_t nreq = D.reqs.size();
      HIPCHK(hipSetDevice(d.ordinal));
      HIPCHK(sd.d_part.reserve(D.total_tiles, 1024));
      HIPCHK(sd.d_seg.reserve(D.fast.size(), 4 * kMaxSegs));
      HIPCHK(sd.h_seg.reserve(D.fast.size(), 4 * kMaxSegs));
      HIPCHK(sd.d_gseg.reserve(D.gsegs.size(), 64));
      HIPCHK(sd.h_gseg.reserve(D.gsegs.size(), 64));
      HIPCHK(sd.d_wrange.reserve(D.ranges.size(), 64));
      HIPCHK(sd.h_wrange.reserve(D.ranges.size(), 64));
      HIPCHK(sd.d_wrange0.reserve(nreq, 64, 1));
      HIPCHK(sd.h_wrange0.reserve(nreq, 64, 1));
      HIPCHK(sd.d_wout.reserve(nreq, 64));
      HIPCHK(sd.h_wout.reserve(nreq, 64));
      const WideBufs b = {sd.d_part.p,   sd.d_seg.p,     sd.h_seg.p,     sd.d_gseg.p, sd.h_gseg.p, sd.d_wrange.p,
                          sd.h_wrange.p, sd.d_wrange0.p, sd.h_wrange0.p, sd.d_wout.p, sd.h_wout.p};
      if ((rc = wide_enqueue(d, D, b)) != P1HIP_OK) return rc;
      C.dev_used[dv] = 1;
      C.parts.push_back({sd.h_wout.p, D.reqs});
      C.wadd.scan_launches += D.launches.size();
      C.wadd.scan_segments += D.fast.size();
      C.wadd.generic_launches += D.gen_tiles ? 1 : 0;
      C.wadd.generic_segments += D.gsegs.size();
      C.wadd.tiles += D.total_tiles;
      C.wadd.nonces += D.nonces;
    }
  // one event per device, after the last copy back
  for (size_t dv = 0; dv < nd; ++dv) {
    if (!C.dev_used[dv]) continue;
    Dev& d = R.devs[dv];
    SlotDev& sd = d.slot[s];
    HIPCHK(hipSetDevice(d.ordinal));
    if (!sd.done) HIPCHK(hipEventCreate(&sd.done));
    HIPCHK(hipEventRecord(sd.done, d.stream));
  }
  return P1HIP_OK;
}

void drain_streams(Runtime& R) {
  const std::string keep = g_err;
  for (Dev& d : R.devs)
    if (d.stream) (void)hipStreamSynchronize(d.stream);
  g_err = keep;
}

int batch_submit_locked(const p1hip_request_t* reqs, size_t n, bool wide, p1hip_ticket_t* ticket) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  const auto t0 = std::chrono::steady_clock::now();
  if (R.slots.Outstanding() >= P1HIP_MAX_INFLIGHT) {
    R.astats.busy++;
    return fail(P1HIP_ERR_BUSY, "P1HIP_MAX_INFLIGHT tickets are outstanding: wait for one first");
  }
  int rc = n ? ensure_init(R) : P1HIP_OK;
  if (rc) return rc;
  const uint64_t t = R.slots.Alloc();
  const int s = R.slots.Holds(t);
  AsyncCall& C = R.calls[s];
  C = AsyncCall();
  // a failure (or a host exception) after the first enqueue leaves nothing
  // in flight in the slot's buffers and no ticket
  auto abandon = [&] {
    drain_streams(R);
    C = AsyncCall();
    R.slots.Release(t);
  };
  try {
    rc = n ? submit_enqueue(R, s, C, reqs, n, wide) : P1HIP_OK;
  } catch (...) {
    abandon();
    throw;
  }
  if (rc != P1HIP_OK) {
    abandon();
    return rc;
  }
  C.submit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  R.astats.submits++;
  R.astats.submit_ms += C.submit_ms;
  R.astats.max_inflight = std::max<uint64_t>(R.astats.max_inflight, (uint64_t)R.slots.Outstanding());
  *ticket = t;
  return P1HIP_OK;
}

int batch_wait_locked(p1hip_ticket_t ticket, p1hip_result_t* out) {
  Runtime& R = rt();
  std::unique_lock<std::mutex> lk(R.mu);
  const auto t0 = std::chrono::steady_clock::now();
  const int s = R.slots.Claim(ticket);
  if (s < 0) return fail(P1HIP_ERR_ARGS, "ticket is unknown, already waited or cancelled");
  AsyncCall& C = R.calls[s];
  // Block on the ticket's events with the mutex released: other threads
  // submit, wait and scan meanwhile.  The slot is claimed, so nobody reuses
  // its buffers, and shutdown_locked lets this thread out before it destroys
  // the events.
  std::vector<hipEvent_t> evs;
  for (size_t dv = 0; dv < C.dev_used.size() && dv < R.devs.size(); ++dv)
    if (C.dev_used[dv]) evs.push_back(R.devs[dv].slot[s].done);
  hipError_t werr = hipSuccess;
  if (!evs.empty()) {
    R.blockers++;
    lk.unlock();
    for (hipEvent_t e : evs) {
      const hipError_t x = hipEventSynchronize(e);
      if (werr == hipSuccess) werr = x;
    }
    lk.lock();
    R.blockers--;
    R.cv.notify_all();
  }
  if (R.slots.Holds(ticket) != s) return fail(P1HIP_ERR_ARGS, "ticket was cancelled by p1hip_shutdown or a re-init");
  auto finish = [&]() -> int {
    if (werr != hipSuccess) return fail(P1HIP_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(werr));
    if (C.n && !out) return fail(P1HIP_ERR_ARGS, "null result array");
    for (const AsyncCall::Part& P : C.parts)
      for (size_t r = 0; r < P.reqs.size(); ++r) {
        const Key kq = finish_key(P.h_out[r]);
        C.res[P.reqs[r]] = p1hip_result_t{kq.h, kq.n};
      }
    // individual route: one by one through the multi-device scan path
    for (const AsyncCall::Indiv& I : C.indiv) {
      const int rc = scan_held(R, (const uint8_t*)I.msg.data(), I.msg.size(), I.lower, I.upper, &C.res[I.idx].hash,
                               &C.res[I.idx].nonce);
      if (rc) return fail(rc, "request " + std::to_string(I.idx) + ": " + g_err);
    }
    return P1HIP_OK;
  };
  // the ticket is spent and the slot free again, whatever happens
  auto release = [&] {
    C = AsyncCall();
    R.slots.Release(ticket);
  };
  int rc;
  try {
    rc = finish();
  } catch (...) {
    drain_streams(R);
    release();
    throw;
  }
  if (rc != P1HIP_OK) {
    drain_streams(R);  // the slot's buffers are idle before the next submit takes them
    release();
    return rc;
  }
  for (size_t i = 0; i < C.n; ++i) out[i] = C.res[i];
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (C.has_b) {
    p1hip_batch_stats_t& S = R.bstats;
    S.calls++;
    S.requests += C.badd.requests;
    S.coalesced += C.badd.coalesced;
    S.individual += C.badd.individual;
    S.empty += C.badd.empty;
    S.launches += C.badd.launches;
    S.tiles += C.badd.tiles;
    S.nonces += C.badd.nonces;
    if (!C.has_w) S.wall_ms += C.submit_ms + ms;
  }
  if (C.has_w) {
    p1hip_wide_stats_t& S = R.wstats;
    S.calls++;
    S.requests += C.wadd.requests;
    S.empty += C.wadd.empty;
    S.small += C.wadd.small;
    S.wide += C.wadd.wide;
    S.individual += C.wadd.individual;
    S.scan_launches += C.wadd.scan_launches;
    S.scan_segments += C.wadd.scan_segments;
    S.generic_launches += C.wadd.generic_launches;
    S.generic_segments += C.wadd.generic_segments;
    S.tiles += C.wadd.tiles;
    S.nonces += C.wadd.nonces;
    S.wall_ms += C.submit_ms + ms;
  }
  R.astats.waits++;
  R.astats.wait_ms += ms;
  release();
  return P1HIP_OK;
}

// ----------------------------------------------------------------------------
// p1hip_reduce_pairs
// ----------------------------------------------------------------------------
int reduce_pairs_locked(const uint64_t* hashes, const uint64_t* nonces, size_t n, uint64_t* out_hash,
                        uint64_t* out_nonce) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  int rc = ensure_init(R);
  if (rc) return rc;
  Dev& d = R.devs[0];
  HIPCHK(hipSetDevice(d.ordinal));
  Key res = {~0ull, ~0ull};
  if (n > (size_t)kMaxLaunchBlocks * kBlock) return fail(P1HIP_ERR_ARGS, "too many pairs");
  if (n) {
    // scratch of exactly this call's size, freed on every exit path (HIPCHK
    // returns early; the stream is synchronised before the normal one)
    DevBuf<uint64_t> dh, dn;
    DevBuf<Key> dp;
    const uint32_t blocks = (uint32_t)((n + kBlock - 1) / kBlock);
    HIPCHK(dh.reserve(n, n));
    HIPCHK(dn.reserve(n, n));
    HIPCHK(dp.reserve(blocks, blocks));
    HIPCHK(hipMemcpyAsync(dh.p, hashes, n * 8, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipMemcpyAsync(dn.p, nonces, n * 8, hipMemcpyHostToDevice, d.stream));
    HIPCHK(launch(d.f_pairs, blocks, kBlock, d.stream, (const uint64_t*)dh.p, (const uint64_t*)dn.p, (uint64_t)n,
                  dp.p));
    HIPCHK(launch(d.f_reduce, 1, kReduceThreads, d.stream, (const Key*)dp.p, blocks, d.d_res.p));
    HIPCHK(hipMemcpyAsync(d.h_res.p, d.d_res.p, sizeof(Key), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    res = d.h_res.p[0];
  }
  res = finish_key(res);
  *out_hash = res.h;
  *out_nonce = res.n;
  return P1HIP_OK;
}

// ----------------------------------------------------------------------------
// p1hip_scan_tiles
// ----------------------------------------------------------------------------
// One share on the first device, routed as scan_held's phase 1 routes it
// (k_scan_small up to P1HIP_SMALL_MAX_NONCES, else run_range with the
// runtime's planner settings), with a TileDump.
int scan_tiles_locked(const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, size_t cap, size_t* count,
                      p1hip_tile_t* tiles, int* route, uint64_t* out_hash, uint64_t* out_nonce) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  int rc = ensure_init(R);
  if (rc) return rc;
  Dev& d = R.devs[0];
  d.replans = 0;
  TileDump dump;
  const bool small = upper - lower < knob(kSmallMaxNoncesKnob);
  rc = small ? run_small(d, msg, msg_len, lower, upper, false, R.profiling, &dump)
             : run_range(d, msg, msg_len, lower, upper, R.profiling, R.min_fast_threads, R.split, R.tabulate, &dump);
  if (rc) return rc;
  *count = dump.map.size();
  for (size_t i = 0; i < dump.map.size() && i < cap; ++i) {
    const TileInfo& T = dump.map[i];
    p1hip_tile_t& o = tiles[i];
    memset(&o, 0, sizeof o);
    o.launch = T.launch;
    o.tile = T.tile;
    o.kind = T.kind;
    o.k = T.k;
    o.nruns = T.nruns;
    for (uint32_t r = 0; r < T.nruns; ++r)
      o.runs[r] = {T.runs[r].first, T.runs[r].stride, T.runs[r].run_len, T.runs[r].count};
    o.hash = dump.part[i].h;
    o.nonce = dump.part[i].n;
  }
  *route = small ? 1 : 0;
  const Key res = finish_key(dump.res);
  *out_hash = res.h;
  *out_nonce = res.n;
  return P1HIP_OK;
}

// ----------------------------------------------------------------------------
// p1hip_scan_below
// ----------------------------------------------------------------------------
// the public header restates below_abi.hpp's constants
static_assert(P1HIP_BELOW_MAX_SLICE == kBelowMaxSliceSparse && P1HIP_BELOW_MAX_SLICE_DENSE == kBelowMaxSliceDense &&
                  P1HIP_BELOW_DENSE_TARGET == kBelowDenseTarget,
              "p1hip.h and below_abi.hpp disagree");

// One launch of k_below_mark on device d: table B up, the kernel, the marks
// back into d.h_marks; synchronises.  Workgroup b of the B.tiles launched
// writes words [4b, 4b + 4) of the 4 * B.tiles reserved, every one of them, so
// the marks are not cleared first.  The buffers are this path's own and grow
// only here, between two synchronised launches of it.
int below_mark(Dev& d, const BelowTable& B, uint64_t target) {
  const size_t nseg = B.T.segs.size(), words = (size_t)B.tiles * kBelowWordsPerTile;
  HIPCHK(hipSetDevice(d.ordinal));
  HIPCHK(d.d_mseg.reserve(nseg, 64));
  HIPCHK(d.h_mseg.reserve(nseg, 64));
  HIPCHK(d.d_marks.reserve(words, 4096));
  HIPCHK(d.h_marks.reserve(words, 4096));
  memcpy(d.h_mseg.p, B.T.segs.data(), nseg * sizeof(BatchSeg));
  HIPCHK(hipMemcpyAsync(d.d_mseg.p, d.h_mseg.p, nseg * sizeof(BatchSeg), hipMemcpyHostToDevice, d.stream));
  HIPCHK(launch(d.f_mark, B.tiles, kBlock, d.stream, (const BatchSeg*)d.d_mseg.p, (uint32_t)nseg, target, d.d_marks.p));
  HIPCHK(hipMemcpyAsync(d.h_marks.p, d.d_marks.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  return P1HIP_OK;
}

// Pass 1 of a sparse slice: [lo, hi] cut across the open devices as p1hip_scan
// cuts it, run_range on each with p1hip_scan's settings -- every device
// enqueued before any is synchronised -- and the tiles whose partial is at or
// below the target turned into pieces (below_plan.hpp).  No combine: the
// partials are all the filter needs.
int below_filter(Runtime& R, const uint8_t* msg, size_t msg_len, uint64_t lo, uint64_t hi, uint64_t target,
                 std::vector<BelowPiece>& pieces, std::vector<Key>& cand_part, p1hip_below_stats_t& add) {
  const size_t nd = R.devs.size();
  std::vector<uint64_t> slo(nd), shi(nd);
  plan_shards(msg, msg_len, lo, hi, (int)nd, slo.data(), shi.data());
  std::vector<TileDump> dumps(nd);
  int rc;
  for (size_t i = 0; i < nd; ++i) {
    if (slo[i] > shi[i]) continue;
    Dev& d = R.devs[i];
    d.replans = 0;
    if ((rc = run_range(d, msg, msg_len, slo[i], shi[i], R.profiling, R.min_fast_threads, R.split, R.tabulate,
                        &dumps[i], false, false)))
      return rc;
    add.scan_nonces += d.ctr.scan_nonces;
    d.acc.scan_launches += d.ctr.scan_launches;
    d.acc.scan_nonces += d.ctr.scan_nonces;
    d.acc.scan_alg_ops += d.ctr.scan_ops;
    d.acc.scan_kernel_ms += d.ctr.scan_ms;
  }
  for (size_t i = 0; i < nd; ++i) {
    if (slo[i] > shi[i]) continue;
    Dev& d = R.devs[i];
    HIPCHK(hipSetDevice(d.ordinal));
    if ((rc = dump_collect(d, d.d_part.p, dumps[i]))) return rc;
    for (size_t t = 0; t < dumps[i].map.size(); ++t)
      if (below_candidate(dumps[i].map[t], dumps[i].part[t], target)) {
        below_tile_pieces(dumps[i].map[t], (uint32_t)cand_part.size(), pieces);
        cand_part.push_back(dumps[i].part[t]);
      }
  }
  return P1HIP_OK;
}

// One p1hip_scan_below with R.mu held by the caller (p1hip_scan_below;
// p1hip_scan_below_batch for its individual requests): the hits go to `res`
// (empty on entry), which holds the whole answer only when the call succeeds.
int scan_below_held(Runtime& R, const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, uint64_t target,
                    size_t cap, std::vector<p1hip_result_t>& res) {
  const auto t0 = std::chrono::steady_clock::now();
  int rc = ensure_init(R);
  if (rc) return rc;
  const int path = (int)knob(kBelowPathKnob);
  const uint64_t max_slice = knob(kBelowMaxSliceKnob);
  p1hip_below_stats_t add{};
  auto run = [&]() -> int {
    std::vector<BelowPiece> pieces;
    std::vector<Key> cand_part;
    std::vector<BelowHit> got;
    BelowTable B;
    for (uint64_t lo = lower;;) {
      const size_t want = cap - res.size();
      const BelowSlice S = below_next_slice(lo, upper, target, want, path, max_slice);
      pieces.clear();
      cand_part.clear();
      got.clear();
      if (S.dense) {
        below_dense_pieces(S.lo, S.hi, pieces);
        add.dense_slices++;
      } else {
        if ((rc = below_filter(R, msg, msg_len, S.lo, S.hi, target, pieces, cand_part, add))) return rc;
        add.sparse_slices++;
        add.candidate_tiles += cand_part.size();
      }
      // the mark launches, on the first device; a dense slice's pieces are in
      // nonce order, so it may stop at the hits still wanted
      for (size_t first = 0; first < pieces.size() && got.size() < (S.dense ? want : ~(size_t)0); first += B.count) {
        std::string err = below_build_table(msg, msg_len, pieces, first, B);
        if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
        if (B.count == 0 || B.tiles == 0) return fail(P1HIP_ERR_HIP, "internal: empty refine table");
        if ((rc = below_mark(R.devs[0], B, target))) return rc;
        add.mark_launches++;
        add.mark_nonces += B.T.nonces;
        err = below_decode(B, pieces, R.devs[0].h_marks.p, target, S.dense ? want - got.size() : ~(size_t)0, got);
        if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
      }
      if (!S.dense) {
        const std::string err = below_check_candidates(cand_part, got);
        if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
        below_sort_hits(got);
      }
      for (size_t i = 0; i < got.size() && res.size() < cap; ++i) res.push_back({got[i].key.h, got[i].key.n});
      add.slices++;
      add.examined += S.hi - S.lo + 1;
      if (res.size() == cap || S.hi == upper) return P1HIP_OK;
      lo = S.hi + 1;
    }
  };
  if ((rc = run()) != P1HIP_OK) {
    // leave nothing in flight behind a failed call: the next one rewrites the pinned staging tables
    const std::string keep = g_err;
    for (Dev& d : R.devs) (void)hipStreamSynchronize(d.stream);
    g_err = keep;
    return rc;
  }
  p1hip_below_stats_t& T = R.lstats;
  T.calls++;
  T.slices += add.slices;
  T.sparse_slices += add.sparse_slices;
  T.dense_slices += add.dense_slices;
  T.examined += add.examined;
  T.scan_nonces += add.scan_nonces;
  T.mark_nonces += add.mark_nonces;
  T.candidate_tiles += add.candidate_tiles;
  T.mark_launches += add.mark_launches;
  T.hits += res.size();
  T.wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return P1HIP_OK;
}

int scan_below_locked(const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, uint64_t target, size_t cap,
                      p1hip_result_t* hits, size_t* found) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  // results are gathered here and copied to `hits` only when the whole call has succeeded
  std::vector<p1hip_result_t> res;
  if (int rc = scan_below_held(R, msg, msg_len, lower, upper, target, cap, res)) return rc;
  for (size_t i = 0; i < res.size(); ++i) hits[i] = res[i];
  *found = res.size();
  return P1HIP_OK;
}

// ----------------------------------------------------------------------------
// p1hip_scan_below_batch
// ----------------------------------------------------------------------------
// the public header restates belowb_abi.hpp's constants
static_assert(P1HIP_BELOW_BATCH_MAX_NONCES == kBelowBatchMaxNonces && P1HIP_BELOW_BATCH_MAX_SLOTS == kBelowBatchMaxSlots,
              "p1hip.h and belowb_abi.hpp disagree");

int below_batch_check(const p1hip_below_request_t* reqs, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    if (!reqs[i].msg && reqs[i].msg_len > 0)
      return fail(P1HIP_ERR_ARGS, "request " + std::to_string(i) + ": msg == NULL with msg_len > 0");
    if (reqs[i].msg_len > P1HIP_MAX_MSG_LEN)
      return fail(P1HIP_ERR_ARGS, "request " + std::to_string(i) + ": msg_len exceeds P1HIP_MAX_MSG_LEN");
  }
  return P1HIP_OK;
}

std::vector<BelowBReq> below_batch_reqs(const p1hip_below_request_t* reqs, size_t n) {
  std::vector<BelowBReq> q(n);
  for (size_t i = 0; i < n; ++i)
    q[i] = {reqs[i].msg, reqs[i].msg_len, reqs[i].lower, reqs[i].upper, reqs[i].target, (uint64_t)reqs[i].cap};
  return q;
}

// Where one launch pair's tables and results lie in its device's buffers
// (elements): segments, targets, the two request tables, counts + indices.
struct BelowBPlace {
  size_t seg0, req0, tab0, out0;
};

// Enqueue launch pair (L, B) on device d's stream: the tables, k_belowb_mark,
// k_belowb_collect.  No copy back (one per device per round follows the
// device's last pair) and no synchronisation.  Workgroup b of the L.tiles
// marked writes words [4b, 4b + 4) of d_qmarks, every one of them, and request
// r's collect workgroup reads only words of its own tiles, so the marks are
// not cleared first; the device's next pair reuses them in stream order.
int below_batch_enqueue(Dev& d, const BelowBLaunch& L, const BelowBTable& B, const BelowBPlace& P) {
  const size_t nseg = B.T.segs.size(), nreq = L.items.size();
  memcpy(d.h_qseg.p + P.seg0, B.T.segs.data(), nseg * sizeof(BatchSeg));
  memcpy(d.h_qtarget.p + P.req0, B.targets.data(), nreq * sizeof(uint64_t));
  memcpy(d.h_qtab.p + P.tab0, B.T.req_tile0.data(), (nreq + 1) * sizeof(uint32_t));
  memcpy(d.h_qtab.p + P.tab0 + nreq + 1, B.req_hit0.data(), (nreq + 1) * sizeof(uint32_t));
  HIPCHK(hipMemcpyAsync(d.d_qseg.p + P.seg0, d.h_qseg.p + P.seg0, nseg * sizeof(BatchSeg), hipMemcpyHostToDevice,
                        d.stream));
  HIPCHK(hipMemcpyAsync(d.d_qtarget.p + P.req0, d.h_qtarget.p + P.req0, nreq * sizeof(uint64_t), hipMemcpyHostToDevice,
                        d.stream));
  HIPCHK(hipMemcpyAsync(d.d_qtab.p + P.tab0, d.h_qtab.p + P.tab0, 2 * (nreq + 1) * sizeof(uint32_t),
                        hipMemcpyHostToDevice, d.stream));
  HIPCHK(launch(d.f_qmark, L.tiles, kBlock, d.stream, (const BatchSeg*)(d.d_qseg.p + P.seg0), (uint32_t)nseg,
                (const uint64_t*)(d.d_qtarget.p + P.req0), d.d_qmarks.p));
  HIPCHK(launch(d.f_qcollect, (uint32_t)nreq, kBlock, d.stream, (const uint64_t*)d.d_qmarks.p,
                (const uint32_t*)(d.d_qtab.p + P.tab0), (const uint32_t*)(d.d_qtab.p + P.tab0 + nreq + 1),
                d.d_qout.p + P.out0 + nreq, d.d_qout.p + P.out0));
  return P1HIP_OK;
}

// The dense launch pairs of one round (p1hip_scan_below_batch;
// p1hip_scan_below_batch_wide for its dense slices): the layout, every pair's
// tables and where they lie in their device's buffers.
struct BelowBRound {
  std::vector<BelowBLaunch> launches;
  std::vector<BelowBTable> tabs;
  std::vector<BelowBPlace> place;
  std::vector<BelowBPlace> need;  // per device: what the round takes of its buffers
};

// Lay the round's items out, build every table of the round, then each
// device's buffers (its stream is idle: every round ends with a
// synchronisation), then the enqueues and one copy back per device.  No
// synchronisation.  `coalesced`: the call's requests BelowBItem::req indexes.
int below_batch_round_enqueue(Runtime& R, const BelowBReq* q, const std::vector<size_t>& coalesced,
                              const std::vector<BelowBItem>& items, BelowBRound& W, p1hip_below_batch_stats_t& add) {
  const int ndev = (int)R.devs.size();
  int rc;
  W.launches = belowb_layout(items, ndev);
  const std::vector<BelowBLaunch>& launches = W.launches;
  W.tabs.resize(launches.size());
  W.place.resize(launches.size());
  W.need.assign((size_t)ndev, BelowBPlace{0, 0, 0, 0});
  std::vector<size_t> max_tiles((size_t)ndev, 0);
  for (size_t l = 0; l < launches.size(); ++l) {
    const BelowBLaunch& L = launches[l];
    const std::string err = belowb_build_table(q, coalesced, items, L, W.tabs[l]);
    if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
    if (L.tiles == 0 || L.tiles > kBatchMaxTiles || L.slots > kBelowBatchMaxSlots)
      return fail(P1HIP_ERR_HIP, "internal: a below batch launch pair outside its limits");
    BelowBPlace& N = W.need[(size_t)L.device];
    W.place[l] = N;
    N.seg0 += W.tabs[l].T.segs.size();
    N.req0 += L.items.size();
    N.tab0 += 2 * (L.items.size() + 1);
    N.out0 += L.items.size() + (size_t)L.slots;
    if (L.tiles > max_tiles[(size_t)L.device]) max_tiles[(size_t)L.device] = L.tiles;
  }
  for (int i = 0; i < ndev; ++i) {
    const BelowBPlace& N = W.need[(size_t)i];
    if (N.req0 == 0) continue;
    Dev& d = R.devs[(size_t)i];
    HIPCHK(hipSetDevice(d.ordinal));
    HIPCHK(d.d_qseg.reserve(N.seg0, 64));
    HIPCHK(d.h_qseg.reserve(N.seg0, 64));
    HIPCHK(d.d_qtarget.reserve(N.req0, 64));
    HIPCHK(d.h_qtarget.reserve(N.req0, 64));
    HIPCHK(d.d_qtab.reserve(N.tab0, 128));
    HIPCHK(d.h_qtab.reserve(N.tab0, 128));
    HIPCHK(d.d_qmarks.reserve(max_tiles[(size_t)i] * kBelowWordsPerTile, 4096));
    HIPCHK(d.d_qout.reserve(N.out0, 1024));
    HIPCHK(d.h_qout.reserve(N.out0, 1024));
  }
  for (size_t l = 0; l < launches.size(); ++l) {
    const BelowBLaunch& L = launches[l];
    Dev& d = R.devs[(size_t)L.device];
    HIPCHK(hipSetDevice(d.ordinal));
    if ((rc = below_batch_enqueue(d, L, W.tabs[l], W.place[l])) != P1HIP_OK) return rc;
    add.launches++;
    add.tiles += L.tiles;
    add.mark_nonces += W.tabs[l].T.nonces;
    // the device's last pair of the round: the one copy back
    if (l + 1 == launches.size() || launches[l + 1].device != L.device) {
      const size_t words = W.need[(size_t)L.device].out0;
      HIPCHK(hipMemcpyAsync(d.h_qout.p, d.d_qout.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
      add.bytes_back += words * sizeof(uint32_t);
    }
  }
  return P1HIP_OK;
}

// Wait for every device that took part in the round.
int below_batch_round_sync(Runtime& R, const BelowBRound& W) {
  for (size_t i = 0; i < W.need.size(); ++i)
    if (W.need[i].req0) {
      Dev& d = R.devs[i];
      HIPCHK(hipSetDevice(d.ordinal));
      HIPCHK(hipStreamSynchronize(d.stream));
    }
  return P1HIP_OK;
}

// Decode what the round's launch pairs returned (belowb_decode's checks):
// each(item, its hits) for every item, in launch order.
template <typename Fn>
int below_batch_round_decode(Runtime& R, const BelowBRound& W, const std::vector<BelowBItem>& items, Fn&& each) {
  std::vector<std::vector<Key>> got;
  for (size_t l = 0; l < W.launches.size(); ++l) {
    const BelowBLaunch& L = W.launches[l];
    const uint32_t* out = R.devs[(size_t)L.device].h_qout.p + W.place[l].out0;
    const std::string err = belowb_decode(W.tabs[l], out + L.items.size(), out, got);
    if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
    for (size_t r = 0; r < L.items.size(); ++r)
      if (int rc = each(items[L.items[r]], got[r])) return rc;
  }
  return P1HIP_OK;
}

int scan_below_batch_locked(const p1hip_below_request_t* reqs, size_t n, const std::vector<size_t>& off,
                            p1hip_result_t* hits, size_t* found) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  const auto t0 = std::chrono::steady_clock::now();
  const int path = (int)knob(kBelowPathKnob);
  const uint64_t max_slice = knob(kBelowMaxSliceKnob);
  const std::vector<BelowBReq> q = below_batch_reqs(reqs, n);
  p1hip_below_batch_stats_t add{};
  std::vector<size_t> coalesced, individual;
  for (size_t i = 0; i < n; ++i) {
    const int route = belowb_route(q[i], path, max_slice);
    if (route == kBelowBCoalesced) coalesced.push_back(i);
    else if (route == kBelowBIndividual) individual.push_back(i);
    else add.empty++;
  }
  // results are gathered here and copied to `hits` only when the whole call has succeeded
  std::vector<std::vector<p1hip_result_t>> res(n);
  int rc;
  auto run = [&]() -> int {
    if (coalesced.empty() && individual.empty()) return P1HIP_OK;  // all empty: no device
    if ((rc = ensure_init(R))) return rc;
    std::vector<BelowBState> st(coalesced.size());
    for (size_t j = 0; j < coalesced.size(); ++j) st[j] = {q[coalesced[j]].lower, 0, false};
    std::vector<BelowBItem> items;
    BelowBRound W;
    for (size_t left = coalesced.size(); left > 0;) {
      const std::string err = belowb_round_items(q.data(), coalesced, st, path, max_slice, items);
      if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
      if ((rc = below_batch_round_enqueue(R, q.data(), coalesced, items, W, add)) != P1HIP_OK) return rc;
      if ((rc = below_batch_round_sync(R, W)) != P1HIP_OK) return rc;
      rc = below_batch_round_decode(R, W, items, [&](const BelowBItem& it, const std::vector<Key>& got) -> int {
        BelowBState& S = st[it.req];
        const size_t i = coalesced[it.req];
        for (const Key& k : got) {
          if (!res[i].empty() && k.n <= res[i].back().nonce)
            return fail(P1HIP_ERR_HIP, "collect check: request " + std::to_string(i) + " has nonces out of order");
          res[i].push_back({k.h, k.n});
        }
        S.found += got.size();
        if (S.found == q[i].cap || it.hi == q[i].upper) {
          S.done = true;
          --left;
        } else {
          S.lo = it.hi + 1;
        }
        return P1HIP_OK;
      });
      if (rc != P1HIP_OK) return rc;
      add.rounds++;
    }
    // The other requests: one by one through p1hip_scan_below's own path.
    for (size_t i : individual)
      if ((rc = scan_below_held(R, q[i].msg, q[i].len, q[i].lower, q[i].upper, q[i].target, (size_t)q[i].cap, res[i])))
        return fail(rc, "request " + std::to_string(i) + ": " + g_err);
    return P1HIP_OK;
  };
  if ((rc = run()) != P1HIP_OK) {
    // leave no launch pair in flight behind a failed call: the next call
    // rewrites the pinned staging tables
    const std::string keep = g_err;
    for (Dev& d : R.devs) (void)hipStreamSynchronize(d.stream);
    g_err = keep;
    return rc;
  }
  for (size_t i = 0; i < n; ++i) {
    for (size_t k = 0; k < res[i].size(); ++k) hits[off[i] + k] = res[i][k];
    found[i] = res[i].size();
    add.hits += res[i].size();
  }
  p1hip_below_batch_stats_t& T = R.qstats;
  T.calls++;
  T.requests += n;
  T.empty += add.empty;
  T.coalesced += coalesced.size();
  T.individual += individual.size();
  T.rounds += add.rounds;
  T.launches += add.launches;
  T.tiles += add.tiles;
  T.mark_nonces += add.mark_nonces;
  T.hits += add.hits;
  T.bytes_back += add.bytes_back;
  T.wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return P1HIP_OK;
}

// p1hip_below_collect (test hook): k_belowb_collect alone on the first device,
// in scratch of exactly this call's size, as reduce_pairs_locked's.
int below_collect_locked(const uint64_t* words, const uint32_t* req_tile0, const uint32_t* req_hit0, size_t nreq,
                         uint32_t* idx, uint32_t* count) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  int rc = ensure_init(R);
  if (rc) return rc;
  Dev& d = R.devs[0];
  HIPCHK(hipSetDevice(d.ordinal));
  const size_t nwords = (size_t)req_tile0[nreq] * kBelowWordsPerTile, nslots = req_hit0[nreq];
  DevBuf<uint64_t> dm;
  DevBuf<uint32_t> dt, dx, dc;
  HIPCHK(dm.reserve(nwords + 1, nwords + 1));
  HIPCHK(dt.reserve(2 * (nreq + 1), 2 * (nreq + 1)));
  HIPCHK(dx.reserve(nslots + 1, nslots + 1));
  HIPCHK(dc.reserve(nreq, nreq));
  if (nwords) HIPCHK(hipMemcpyAsync(dm.p, words, nwords * sizeof(uint64_t), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dt.p, req_tile0, (nreq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dt.p + nreq + 1, req_hit0, (nreq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
  // only for the hook: a slot the kernel leaves alone reads UINT32_MAX
  HIPCHK(hipMemsetAsync(dx.p, 0xff, (nslots + 1) * sizeof(uint32_t), d.stream));
  HIPCHK(launch(d.f_qcollect, (uint32_t)nreq, kBlock, d.stream, (const uint64_t*)dm.p, (const uint32_t*)dt.p,
                (const uint32_t*)(dt.p + nreq + 1), dx.p, dc.p));
  std::vector<uint32_t> hx(nslots), hc(nreq);
  if (nslots) HIPCHK(hipMemcpyAsync(hx.data(), dx.p, nslots * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipMemcpyAsync(hc.data(), dc.p, nreq * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  for (size_t i = 0; i < nslots; ++i) idx[i] = hx[i];
  for (size_t i = 0; i < nreq; ++i) count[i] = hc[i];
  return P1HIP_OK;
}

// ----------------------------------------------------------------------------
// p1hip_scan_below_batch_wide
// ----------------------------------------------------------------------------
static_assert(P1HIP_BELOW_WIDE_MAX_NONCES == kWideMaxNonces, "p1hip.h and wide_plan.hpp disagree");

// One device's part of one group of sparse slices: the filter's tables, what
// phase B refines and the mark launch in flight.
struct BelowWWork {
  BelowWFilter F;
  BelowWRefine X;
  std::vector<char> known;  // per candidate: its partial is already in X (the host filter's)
  std::vector<BelowHit> hits;
  size_t next = 0;  // first piece of X not yet marked
  BelowTable B;     // the table in flight
  std::vector<uint64_t> targets;
  bool busy = false;
};

// Phase A of device d: the tables, one k_batch_scan for the generic pieces, the
// shared k_scan launches (wide_enqueue's, in the same buffers: d_part, d_seg and
// the ticket are p1hip_scan's, d_bseg the batch's, d_wrange the wide call's),
// then k_beloww_filter and the copy back of one count per request and its
// candidate slots.  No synchronisation.  The stream may still run the round's
// dense launch pairs, which use none of the buffers grown here.
int beloww_enqueue(Dev& d, const WideDevice& D, const BelowWFilter& F, p1hip_below_wide_stats_t& add) {
  const size_t nreq = D.reqs.size(), nslot = F.req_slot0[nreq];
  HIPCHK(hipSetDevice(d.ordinal));
  HIPCHK(d.d_part.reserve(D.total_tiles, 1));
  HIPCHK(d.d_seg.reserve(D.fast.size(), 4 * kMaxSegs));
  HIPCHK(d.h_seg.reserve(D.fast.size(), 4 * kMaxSegs));
  HIPCHK(d.d_bseg.reserve(D.gsegs.size(), 64));
  HIPCHK(d.h_bseg.reserve(D.gsegs.size(), 64));
  HIPCHK(d.d_wrange.reserve(D.ranges.size(), 64));
  HIPCHK(d.h_wrange.reserve(D.ranges.size(), 64));
  HIPCHK(d.d_ftab.reserve(2 * (nreq + 1), 128));
  HIPCHK(d.h_ftab.reserve(2 * (nreq + 1), 128));
  HIPCHK(d.d_ftarget.reserve(nreq, 64));
  HIPCHK(d.h_ftarget.reserve(nreq, 64));
  HIPCHK(d.d_fcand.reserve(nreq + nslot, 1024));
  HIPCHK(d.h_fcand.reserve(nreq + nslot, 1024));
  for (const WideLaunch& W : D.launches) {
    const std::string err = wide_fill_launch(D, W, d.h_seg.p + W.first);
    if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
  }
  if (!D.fast.empty())
    HIPCHK(hipMemcpyAsync(d.d_seg.p, d.h_seg.p, D.fast.size() * sizeof(Segment), hipMemcpyHostToDevice, d.stream));
  memcpy(d.h_wrange.p, D.ranges.data(), D.ranges.size() * sizeof(WideRange));
  memcpy(d.h_ftab.p, D.req_range0.data(), (nreq + 1) * sizeof(uint32_t));
  memcpy(d.h_ftab.p + nreq + 1, F.req_slot0.data(), (nreq + 1) * sizeof(uint32_t));
  memcpy(d.h_ftarget.p, F.targets.data(), nreq * sizeof(uint64_t));
  HIPCHK(hipMemcpyAsync(d.d_wrange.p, d.h_wrange.p, D.ranges.size() * sizeof(WideRange), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(d.d_ftab.p, d.h_ftab.p, 2 * (nreq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(d.d_ftarget.p, d.h_ftarget.p, nreq * sizeof(uint64_t), hipMemcpyHostToDevice, d.stream));
  if (D.gen_tiles) {
    memcpy(d.h_bseg.p, D.gsegs.data(), D.gsegs.size() * sizeof(BatchSeg));
    HIPCHK(hipMemcpyAsync(d.d_bseg.p, d.h_bseg.p, D.gsegs.size() * sizeof(BatchSeg), hipMemcpyHostToDevice, d.stream));
    HIPCHK(launch(d.f_bscan, D.gen_tiles, kBlock, d.stream, (const BatchSeg*)d.d_bseg.p, (uint32_t)D.gsegs.size(),
                  (Key*)(d.d_part.p + D.gen_tile0)));
  }
  for (const WideLaunch& W : D.launches) {
#ifdef P1_STATIC_GRID
    HIPCHK(launch(d.f_scan, W.tiles, kBlock, d.stream, (const Segment*)(d.d_seg.p + W.first), (uint32_t)W.count,
                  (Key*)(d.d_part.p + W.tile0)));
#else
    HIPCHK(launch(d.f_scan, scan_grid_for(d, W.tiles), kBlock, d.stream, (const Segment*)(d.d_seg.p + W.first),
                  (uint32_t)W.count, (Key*)(d.d_part.p + W.tile0), (uint32_t)W.tiles, d.d_scan_ticket.p));
#endif
  }
  HIPCHK(launch(d.f_wfilter, (uint32_t)nreq, kBlock, d.stream, (const Key*)d.d_part.p, (const WideRange*)d.d_wrange.p,
                (const uint32_t*)d.d_ftab.p, (const uint64_t*)d.d_ftarget.p, (const uint32_t*)(d.d_ftab.p + nreq + 1),
                d.d_fcand.p + nreq, d.d_fcand.p));
  HIPCHK(hipMemcpyAsync(d.h_fcand.p, d.d_fcand.p, (nreq + nslot) * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
  uint64_t fast_nonces = 0;
  for (const WideFast& f : D.fast) fast_nonces += D.plans[f.req].launches[f.piece].nonces;
  d.acc.scan_launches += D.launches.size();
  d.acc.scan_nonces += fast_nonces;
  add.scan_launches += D.launches.size();
  add.scan_segments += D.fast.size();
  add.generic_launches += D.gen_tiles ? 1 : 0;
  add.scan_nonces += D.nonces;
  add.filter_launches++;
  add.bytes_back += (nreq + nslot) * sizeof(uint32_t);
  return P1HIP_OK;
}

// After phase A of device d is synchronised: every request's candidates into
// W.X.  A request that reports more candidates than it has slots is filtered
// here instead: its ranges of the partial array, which are still on the device,
// are copied back and walked with the kernel's own per-thread function.  The
// partials of the other candidates are fetched (16 bytes each, neighbours in
// one copy) into d.h_fpart; that copy is enqueued, not waited for.
int beloww_candidates(Dev& d, const std::vector<size_t>& live, const std::vector<BelowWItem>& sparse,
                      const BelowWGroup& G, size_t dv, BelowWWork& W, p1hip_below_wide_stats_t& add) {
  const WideDevice& D = G.Y.devs[dv];
  const size_t nreq = D.reqs.size();
  HIPCHK(hipSetDevice(d.ordinal));
  const uint32_t* count = d.h_fcand.p;
  const uint32_t* cand = d.h_fcand.p + nreq;
  std::vector<Key> hpart;
  std::vector<uint32_t> idx;
  for (uint32_t r = 0; r < (uint32_t)nreq; ++r) {
    const size_t i = live[sparse[G.members[D.reqs[r]]].req];
    const uint32_t s0 = W.F.req_slot0[r], slots = W.F.req_slot0[r + 1] - s0;
    const size_t before = W.X.cand_req.size();
    const bool overflow = count[r] > slots;
    std::string err;
    if (!overflow) {
      err = beloww_add_candidates(D, W.F, r, i, cand + s0, count[r], W.X);
    } else {
      add.slot_overflows++;
      hpart.resize(D.total_tiles);
      for (uint32_t j = D.req_range0[r]; j < D.req_range0[r + 1]; ++j) {
        const WideRange Rg = D.ranges[j];
        HIPCHK(hipMemcpyAsync(hpart.data() + Rg.tile0, d.d_part.p + Rg.tile0, (size_t)Rg.ntiles * sizeof(Key),
                              hipMemcpyDeviceToHost, d.stream));
        add.bytes_back += (uint64_t)Rg.ntiles * sizeof(Key);
      }
      HIPCHK(hipStreamSynchronize(d.stream));
      idx.clear();
      for (uint32_t j = D.req_range0[r]; j < D.req_range0[r + 1]; ++j) {
        const WideRange Rg = D.ranges[j];
        for (uint32_t t = 0; t < Rg.ntiles; ++t) {
          uint32_t tile;
          if (beloww_thread(hpart.data(), Rg, 0, t, W.F.targets[r], &tile)) idx.push_back(tile);
        }
      }
      if (idx.size() != count[r])
        return fail(P1HIP_ERR_HIP, "filter check: request " + std::to_string(i) + " reports " + std::to_string(count[r]) +
                                       " candidates, its partials hold " + std::to_string(idx.size()));
      err = beloww_add_candidates(D, W.F, r, i, idx.data(), (uint32_t)idx.size(), W.X);
    }
    if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
    W.known.resize(W.X.cand_req.size(), overflow);
    if (overflow)
      for (size_t c = before; c < W.X.cand_req.size(); ++c) W.X.cand_part[c] = hpart[W.X.cand_tile[c]];
  }
  const size_t ncand = W.X.cand_req.size();
  add.candidate_tiles += ncand;
  HIPCHK(d.h_fpart.reserve(ncand, 64));
  for (size_t c = 0; c < ncand;) {
    size_t e = c + 1;
    if (!W.known[c]) {
      while (e < ncand && !W.known[e] && W.X.cand_tile[e] == W.X.cand_tile[e - 1] + 1) ++e;
      HIPCHK(hipMemcpyAsync(d.h_fpart.p + c, d.d_part.p + W.X.cand_tile[c], (e - c) * sizeof(Key), hipMemcpyDeviceToHost,
                            d.stream));
      add.bytes_back += (e - c) * sizeof(Key);
    }
    c = e;
  }
  return P1HIP_OK;
}

// Phase B of device d, one step: the k_belowb_mark table that starts at piece
// W.next, the kernel, the marks back whole.  No synchronisation.  The buffers
// are this path's own; the stream runs nothing that uses them.
int beloww_mark_enqueue(Dev& d, const BelowBReq* q, BelowWWork& W, p1hip_below_wide_stats_t& add) {
  const std::string err = beloww_build_table(q, W.X, W.next, W.B, W.targets);
  if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
  if (W.B.count == 0 || W.B.tiles == 0) return fail(P1HIP_ERR_HIP, "internal: empty refine table");
  const size_t nseg = W.B.T.segs.size(), words = (size_t)W.B.tiles * kBelowWordsPerTile;
  HIPCHK(hipSetDevice(d.ordinal));
  HIPCHK(d.d_fseg.reserve(nseg, 64));
  HIPCHK(d.h_fseg.reserve(nseg, 64));
  HIPCHK(d.d_fmtarget.reserve(W.B.count, 64));
  HIPCHK(d.h_fmtarget.reserve(W.B.count, 64));
  HIPCHK(d.d_fmarks.reserve(words, 4096));
  HIPCHK(d.h_fmarks.reserve(words, 4096));
  memcpy(d.h_fseg.p, W.B.T.segs.data(), nseg * sizeof(BatchSeg));
  memcpy(d.h_fmtarget.p, W.targets.data(), W.B.count * sizeof(uint64_t));
  HIPCHK(hipMemcpyAsync(d.d_fseg.p, d.h_fseg.p, nseg * sizeof(BatchSeg), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(d.d_fmtarget.p, d.h_fmtarget.p, W.B.count * sizeof(uint64_t), hipMemcpyHostToDevice, d.stream));
  HIPCHK(launch(d.f_qmark, W.B.tiles, kBlock, d.stream, (const BatchSeg*)d.d_fseg.p, (uint32_t)nseg,
                (const uint64_t*)d.d_fmtarget.p, d.d_fmarks.p));
  HIPCHK(hipMemcpyAsync(d.h_fmarks.p, d.d_fmarks.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
  W.busy = true;
  add.mark_launches++;
  add.mark_tiles += W.B.tiles;
  add.mark_nonces += W.B.T.nonces;
  add.bytes_back += words * sizeof(uint64_t);
  return P1HIP_OK;
}

// The routes of a call and the states of its live (coalesced and filtered) requests.
void beloww_routes(const std::vector<BelowBReq>& q, int path, uint64_t max_slice, std::vector<int>& route,
                   std::vector<size_t>& live, std::vector<BelowWState>& st) {
  route.resize(q.size());
  for (size_t i = 0; i < q.size(); ++i) {
    route[i] = beloww_route(q[i], path, max_slice);
    if (route[i] == kBelowWCoalesced || route[i] == kBelowWFiltered) {
      live.push_back(i);
      st.push_back(beloww_state(q[i], route[i], path, max_slice));
    }
  }
}

int scan_below_batch_wide_locked(const p1hip_below_request_t* reqs, size_t n, const std::vector<size_t>& off,
                                 p1hip_result_t* hits, size_t* found) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  const auto t0 = std::chrono::steady_clock::now();
  const int path = (int)knob(kBelowPathKnob);
  const uint64_t max_slice = knob(kBelowMaxSliceKnob);
  const uint32_t max_segs = (uint32_t)knob(kWideMaxSegsKnob);
  const uint64_t floor = knob(kWideMinFastThreadsKnob), max_slots = knob(kBelowWideMaxSlotsKnob);
  const std::vector<BelowBReq> q = below_batch_reqs(reqs, n);
  p1hip_below_wide_stats_t add{};
  std::vector<int> route;
  std::vector<size_t> live, individual;
  std::vector<BelowWState> st;
  beloww_routes(q, path, max_slice, route, live, st);
  for (size_t i = 0; i < n; ++i) {
    add.empty += route[i] == kBelowWEmpty;
    add.coalesced += route[i] == kBelowWCoalesced;
    add.filtered += route[i] == kBelowWFiltered;
    if (route[i] == kBelowWIndividual) individual.push_back(i);
  }
  // results are gathered here and copied to `hits` only when the whole call has succeeded
  std::vector<std::vector<p1hip_result_t>> res(n);
  int rc;
  // the hits got[0 .. ngot) (in increasing nonce) of live request j, whose slice ended at `hi`
  size_t left = live.size();
  auto take = [&](size_t j, uint64_t hi, const Key* got, size_t ngot) -> int {
    const size_t i = live[j];
    for (size_t k = 0; k < ngot; ++k) {
      if (!res[i].empty() && got[k].n <= res[i].back().nonce)
        return fail(P1HIP_ERR_HIP, "collect check: request " + std::to_string(i) + " has nonces out of order");
      res[i].push_back({got[k].h, got[k].n});
    }
    st[j].found += ngot;
    if (st[j].found == q[i].cap || hi == q[i].upper) {
      st[j].done = true;
      --left;
    } else {
      st[j].lo = hi + 1;
    }
    return P1HIP_OK;
  };
  auto run = [&]() -> int {
    if (live.empty() && individual.empty()) return P1HIP_OK;  // all empty: no device
    if ((rc = ensure_init(R))) return rc;
    const int ndev = (int)R.devs.size();
    std::vector<BelowBItem> dense;
    std::vector<BelowWItem> sparse;
    BelowBRound DR;
    BelowWGroup G;
    std::vector<BelowWWork> work;
    std::vector<std::vector<Key>> got(n);
    while (left > 0) {
      std::string err = beloww_round_items(q.data(), live, st, path, max_slice, dense, sparse);
      if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
      // the dense slices: p1hip_scan_below_batch's launch pairs, decoded at the end of the round
      if (!dense.empty()) {
        p1hip_below_batch_stats_t dadd{};
        if ((rc = below_batch_round_enqueue(R, q.data(), live, dense, DR, dadd)) != P1HIP_OK) return rc;
        add.mark_launches += dadd.launches;
        add.mark_tiles += dadd.tiles;
        add.mark_nonces += dadd.mark_nonces;
        add.bytes_back += dadd.bytes_back;
      }
      // the sparse slices, group after group
      std::vector<size_t> pending(sparse.size());
      for (size_t s = 0; s < sparse.size(); ++s) pending[s] = s;
      while (!pending.empty()) {
        err = beloww_next_group(q.data(), live, sparse, pending, ndev, max_segs, floor, R.split, kWideMaxTiles, G);
        if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
        add.groups++;
        work.clear();
        work.resize((size_t)ndev);
        // phase A: every device enqueued before any is synchronised
        for (int dv = 0; dv < ndev; ++dv) {
          if (G.Y.devs[(size_t)dv].reqs.empty()) continue;
          err = beloww_filter_tables(q.data(), live, sparse, G, (size_t)dv, max_slots, work[(size_t)dv].F);
          if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
          if ((rc = beloww_enqueue(R.devs[(size_t)dv], G.Y.devs[(size_t)dv], work[(size_t)dv].F, add)) != P1HIP_OK) return rc;
        }
        for (int dv = 0; dv < ndev; ++dv) {
          if (G.Y.devs[(size_t)dv].reqs.empty()) continue;
          Dev& d = R.devs[(size_t)dv];
          HIPCHK(hipSetDevice(d.ordinal));
          HIPCHK(hipStreamSynchronize(d.stream));
          if ((rc = beloww_candidates(d, live, sparse, G, (size_t)dv, work[(size_t)dv], add)) != P1HIP_OK) return rc;
        }
        // phase B: one mark launch per device at a time, on the requests' own device
        for (bool any = true; any;) {
          any = false;
          for (int dv = 0; dv < ndev; ++dv) {
            BelowWWork& W = work[(size_t)dv];
            if (W.next >= W.X.pieces.size()) continue;
            if ((rc = beloww_mark_enqueue(R.devs[(size_t)dv], q.data(), W, add)) != P1HIP_OK) return rc;
            any = true;
          }
          for (int dv = 0; dv < ndev; ++dv) {
            BelowWWork& W = work[(size_t)dv];
            if (!W.busy) continue;
            Dev& d = R.devs[(size_t)dv];
            HIPCHK(hipSetDevice(d.ordinal));
            HIPCHK(hipStreamSynchronize(d.stream));
            W.busy = false;
            err = beloww_decode(W.B, W.X, d.h_fmarks.p, W.targets, W.hits);
            if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
            W.next += W.B.count;
          }
        }
        for (int dv = 0; dv < ndev; ++dv) {
          const WideDevice& D = G.Y.devs[(size_t)dv];
          if (D.reqs.empty()) continue;
          BelowWWork& W = work[(size_t)dv];
          for (size_t c = 0; c < W.X.cand_req.size(); ++c)
            if (!W.known[c]) W.X.cand_part[c] = R.devs[(size_t)dv].h_fpart.p[c];
          err = beloww_check_parts(q.data(), W.X);
          if (err.empty()) err = beloww_finish(W.X, W.hits);
          if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
          for (const BelowHit& h : W.hits) got[W.X.cand_req[h.cand]].push_back(h.key);
          for (size_t r = 0; r < D.reqs.size(); ++r) {
            const BelowWItem& it = sparse[G.members[D.reqs[r]]];
            std::vector<Key>& mine = got[live[it.req]];
            if ((rc = take(it.req, it.hi, mine.data(), (size_t)std::min<uint64_t>(it.want, mine.size()))) != P1HIP_OK)
              return rc;
            mine.clear();
          }
        }
      }
      if (!dense.empty()) {
        if ((rc = below_batch_round_sync(R, DR)) != P1HIP_OK) return rc;
        rc = below_batch_round_decode(R, DR, dense, [&](const BelowBItem& it, const std::vector<Key>& hs) -> int {
          return take(it.req, it.hi, hs.data(), hs.size());
        });
        if (rc != P1HIP_OK) return rc;
      }
      add.rounds++;
    }
    // The other requests: one by one through p1hip_scan_below's own path.
    for (size_t i : individual)
      if ((rc = scan_below_held(R, q[i].msg, q[i].len, q[i].lower, q[i].upper, q[i].target, (size_t)q[i].cap, res[i])))
        return fail(rc, "request " + std::to_string(i) + ": " + g_err);
    return P1HIP_OK;
  };
  if ((rc = run()) != P1HIP_OK) {
    // leave nothing in flight behind a failed call: the next call rewrites the pinned staging tables
    const std::string keep = g_err;
    for (Dev& d : R.devs) (void)hipStreamSynchronize(d.stream);
    g_err = keep;
    return rc;
  }
  for (size_t i = 0; i < n; ++i) {
    for (size_t k = 0; k < res[i].size(); ++k) hits[off[i] + k] = res[i][k];
    found[i] = res[i].size();
    add.hits += res[i].size();
  }
  p1hip_below_wide_stats_t& T = R.fstats;
  T.calls++;
  T.requests += n;
  T.empty += add.empty;
  T.coalesced += add.coalesced;
  T.filtered += add.filtered;
  T.individual += individual.size();
  T.rounds += add.rounds;
  T.groups += add.groups;
  T.scan_launches += add.scan_launches;
  T.scan_segments += add.scan_segments;
  T.generic_launches += add.generic_launches;
  T.scan_nonces += add.scan_nonces;
  T.filter_launches += add.filter_launches;
  T.candidate_tiles += add.candidate_tiles;
  T.slot_overflows += add.slot_overflows;
  T.mark_launches += add.mark_launches;
  T.mark_tiles += add.mark_tiles;
  T.mark_nonces += add.mark_nonces;
  T.hits += add.hits;
  T.bytes_back += add.bytes_back;
  T.wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return P1HIP_OK;
}

// p1hip_below_filter (test hook): k_beloww_filter alone on the first device, in
// scratch of exactly this call's size, as below_collect_locked's.
int below_filter_locked(const uint64_t* part_hash, const uint64_t* part_nonce, size_t ntiles, const uint32_t* range_tile0,
                        const uint32_t* range_ntiles, const uint32_t* req_range0, const uint64_t* targets,
                        const uint32_t* req_slot0, size_t nreq, uint32_t* cand, uint32_t* count) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  int rc = ensure_init(R);
  if (rc) return rc;
  Dev& d = R.devs[0];
  HIPCHK(hipSetDevice(d.ordinal));
  const size_t nrange = req_range0[nreq], nslot = req_slot0[nreq];
  std::vector<Key> hp(ntiles);
  for (size_t t = 0; t < ntiles; ++t) hp[t] = Key{part_hash[t], part_nonce[t]};
  std::vector<WideRange> hr(nrange);
  for (size_t j = 0; j < nrange; ++j) hr[j] = WideRange{range_tile0[j], range_ntiles[j]};
  DevBuf<Key> dp;
  DevBuf<WideRange> dr;
  DevBuf<uint64_t> dt;
  DevBuf<uint32_t> dtab, dx, dc;
  HIPCHK(dp.reserve(ntiles + 1, ntiles + 1));
  HIPCHK(dr.reserve(nrange + 1, nrange + 1));
  HIPCHK(dt.reserve(nreq, nreq));
  HIPCHK(dtab.reserve(2 * (nreq + 1), 2 * (nreq + 1)));
  HIPCHK(dx.reserve(nslot + 1, nslot + 1));
  HIPCHK(dc.reserve(nreq, nreq));
  if (ntiles) HIPCHK(hipMemcpyAsync(dp.p, hp.data(), ntiles * sizeof(Key), hipMemcpyHostToDevice, d.stream));
  if (nrange) HIPCHK(hipMemcpyAsync(dr.p, hr.data(), nrange * sizeof(WideRange), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dt.p, targets, nreq * sizeof(uint64_t), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dtab.p, req_range0, (nreq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
  HIPCHK(hipMemcpyAsync(dtab.p + nreq + 1, req_slot0, (nreq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
  // only for the hook: a slot the kernel leaves alone reads UINT32_MAX
  HIPCHK(hipMemsetAsync(dx.p, 0xff, (nslot + 1) * sizeof(uint32_t), d.stream));
  HIPCHK(launch(d.f_wfilter, (uint32_t)nreq, kBlock, d.stream, (const Key*)dp.p, (const WideRange*)dr.p,
                (const uint32_t*)dtab.p, (const uint64_t*)dt.p, (const uint32_t*)(dtab.p + nreq + 1), dx.p, dc.p));
  std::vector<uint32_t> hx(nslot), hc(nreq);
  if (nslot) HIPCHK(hipMemcpyAsync(hx.data(), dx.p, nslot * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipMemcpyAsync(hc.data(), dc.p, nreq * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
  for (size_t i = 0; i < nslot; ++i) cand[i] = hx[i];
  for (size_t i = 0; i < nreq; ++i) count[i] = hc[i];
  return P1HIP_OK;
}

}  // namespace

// ----------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------
extern "C" {

int p1hip_init(int want_devices, int* got_devices) {
  if (got_devices) *got_devices = 0;
  return guarded([&]() {
    Runtime& R = rt();
    std::lock_guard<std::mutex> g(R.mu);
    int count = 0;
    if (int rc = device_count(&count)) return rc;
    int n = want_devices <= 0 ? count : want_devices;
    if (n > count) return fail(P1HIP_ERR_NO_DEVICE, "asked for more devices than visible");
    std::vector<int> ords;
    for (int i = 0; i < n; ++i) ords.push_back(i);
    int rc = init_locked(R, ords);
    if (got_devices) *got_devices = rc == 0 ? (int)R.devs.size() : 0;
    return rc;
  });
}

int p1hip_init_devices(const int* ordinals, int n) {
  if (!ordinals || n <= 0) return fail(P1HIP_ERR_ARGS, "empty device list");
  return guarded([&]() {
    Runtime& R = rt();
    std::lock_guard<std::mutex> g(R.mu);
    return init_locked(R, std::vector<int>(ordinals, ordinals + n));
  });
}

int p1hip_device_count(void) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  return (int)R.devs.size();
}

int p1hip_scan(const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
               uint64_t* out_nonce) {
  if (!out_hash || !out_nonce) return fail(P1HIP_ERR_ARGS, "null output pointer");
  if (!msg && msg_len > 0) return fail(P1HIP_ERR_ARGS, "msg == NULL with msg_len > 0");
  if (msg_len > P1HIP_MAX_MSG_LEN) return fail(P1HIP_ERR_ARGS, "msg_len exceeds P1HIP_MAX_MSG_LEN");
  return guarded([&]() { return scan_locked(msg, msg_len, lower, upper, out_hash, out_nonce); });
}

int p1hip_scan_tiles(const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, size_t cap, size_t* count,
                     p1hip_tile_t* tiles, int* route, uint64_t* out_hash, uint64_t* out_nonce) {
  if (!count || !route || !out_hash || !out_nonce || (!tiles && cap > 0))
    return fail(P1HIP_ERR_ARGS, "null output pointer");
  if (!msg && msg_len > 0) return fail(P1HIP_ERR_ARGS, "msg == NULL with msg_len > 0");
  if (msg_len > P1HIP_MAX_MSG_LEN) return fail(P1HIP_ERR_ARGS, "msg_len exceeds P1HIP_MAX_MSG_LEN");
  if (lower > upper) return fail(P1HIP_ERR_ARGS, "empty range");
  if (upper - lower > 0xffffffffull) return fail(P1HIP_ERR_ARGS, "more than 2^32 nonces");
  return guarded(
      [&]() { return scan_tiles_locked(msg, msg_len, lower, upper, cap, count, tiles, route, out_hash, out_nonce); });
}

int p1hip_scan_below(const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, uint64_t target, size_t cap,
                     p1hip_result_t* hits, size_t* found) {
  if (!found || (!hits && cap > 0)) return fail(P1HIP_ERR_ARGS, "null output pointer");
  if (!msg && msg_len > 0) return fail(P1HIP_ERR_ARGS, "msg == NULL with msg_len > 0");
  if (msg_len > P1HIP_MAX_MSG_LEN) return fail(P1HIP_ERR_ARGS, "msg_len exceeds P1HIP_MAX_MSG_LEN");
  if (lower > upper || cap == 0) {
    *found = 0;
    return P1HIP_OK;
  }
  return guarded([&]() { return scan_below_locked(msg, msg_len, lower, upper, target, cap, hits, found); });
}

int p1hip_get_below_stats(p1hip_below_stats_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null stats pointer");
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  *out = R.lstats;
  return P1HIP_OK;
}

int p1hip_scan_below_batch(const p1hip_below_request_t* reqs, size_t n, p1hip_result_t* hits, size_t hits_len,
                           size_t* found) {
  if (n == 0) return P1HIP_OK;
  if (!reqs || !found) return fail(P1HIP_ERR_ARGS, "null request or found array");
  return guarded([&]() {
    if (int rc = below_batch_check(reqs, n)) return rc;
    std::vector<size_t> off(n);
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
      off[i] = total;
      if (__builtin_add_overflow(total, reqs[i].cap, &total))
        return fail(P1HIP_ERR_ARGS, "request " + std::to_string(i) + ": the sum of the caps overflows");
    }
    if (total > hits_len)
      return fail(P1HIP_ERR_ARGS, "the caps add up to " + std::to_string(total) + ", hits_len is " + std::to_string(hits_len));
    if (!hits && total > 0) return fail(P1HIP_ERR_ARGS, "null hits array");
    return scan_below_batch_locked(reqs, n, off, hits, found);
  });
}

int p1hip_below_batch_layout(const p1hip_below_request_t* reqs, size_t n, int ndev, int32_t* route, int32_t* device,
                             uint32_t* tiles) {
  if (ndev <= 0) return fail(P1HIP_ERR_ARGS, "ndev <= 0");
  if (n == 0) return P1HIP_OK;
  if (!reqs || !route || !device || !tiles) return fail(P1HIP_ERR_ARGS, "null request or output array");
  return guarded([&]() {
    if (int rc = below_batch_check(reqs, n)) return rc;
    const int path = (int)knob(kBelowPathKnob);
    const uint64_t max_slice = knob(kBelowMaxSliceKnob);
    const std::vector<BelowBReq> q = below_batch_reqs(reqs, n);
    std::vector<size_t> coalesced;
    for (size_t i = 0; i < n; ++i) {
      route[i] = belowb_route(q[i], path, max_slice);
      device[i] = -1;
      tiles[i] = 0;
      if (route[i] == kBelowBCoalesced) coalesced.push_back(i);
    }
    std::vector<BelowBState> st(coalesced.size());
    for (size_t j = 0; j < coalesced.size(); ++j) st[j] = {q[coalesced[j]].lower, 0, false};
    std::vector<BelowBItem> items;
    const std::string err = belowb_round_items(q.data(), coalesced, st, path, max_slice, items);
    if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
    for (const BelowBLaunch& L : belowb_layout(items, ndev))
      for (size_t it : L.items) {
        device[coalesced[items[it].req]] = L.device;
        tiles[coalesced[items[it].req]] = items[it].tiles;
      }
    return P1HIP_OK;
  });
}

int p1hip_get_below_batch_stats(p1hip_below_batch_stats_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null stats pointer");
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  *out = R.qstats;
  return P1HIP_OK;
}

int p1hip_below_collect(const uint64_t* words, const uint32_t* req_tile0, const uint32_t* req_hit0, size_t nreq,
                        uint32_t* idx, uint32_t* count) {
  if (nreq == 0) return P1HIP_OK;
  if (!req_tile0 || !req_hit0 || !count) return fail(P1HIP_ERR_ARGS, "null table or count array");
  if (nreq > kBatchMaxTiles) return fail(P1HIP_ERR_ARGS, "too many requests");
  // the kernel trusts its tables: every bound it relies on is checked here
  if (req_tile0[0] != 0 || req_hit0[0] != 0) return fail(P1HIP_ERR_ARGS, "a request table does not start at 0");
  for (size_t r = 0; r < nreq; ++r)
    if (req_tile0[r + 1] < req_tile0[r] || req_hit0[r + 1] < req_hit0[r])
      return fail(P1HIP_ERR_ARGS, "request " + std::to_string(r) + ": a request table falls");
  if (req_tile0[nreq] > kBatchMaxTiles || req_hit0[nreq] > kBelowBatchMaxSlots)
    return fail(P1HIP_ERR_ARGS, "more than 2^20 tiles or 2^22 slots");
  if ((!words && req_tile0[nreq] > 0) || (!idx && req_hit0[nreq] > 0)) return fail(P1HIP_ERR_ARGS, "null words or idx array");
  return guarded([&]() { return below_collect_locked(words, req_tile0, req_hit0, nreq, idx, count); });
}

int p1hip_scan_below_batch_wide(const p1hip_below_request_t* reqs, size_t n, p1hip_result_t* hits, size_t hits_len,
                                size_t* found) {
  if (n == 0) return P1HIP_OK;
  if (!reqs || !found) return fail(P1HIP_ERR_ARGS, "null request or found array");
  return guarded([&]() {
    if (int rc = below_batch_check(reqs, n)) return rc;
    std::vector<size_t> off(n);
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
      off[i] = total;
      if (__builtin_add_overflow(total, reqs[i].cap, &total))
        return fail(P1HIP_ERR_ARGS, "request " + std::to_string(i) + ": the sum of the caps overflows");
    }
    if (total > hits_len)
      return fail(P1HIP_ERR_ARGS, "the caps add up to " + std::to_string(total) + ", hits_len is " + std::to_string(hits_len));
    if (!hits && total > 0) return fail(P1HIP_ERR_ARGS, "null hits array");
    return scan_below_batch_wide_locked(reqs, n, off, hits, found);
  });
}

int p1hip_below_wide_layout(const p1hip_below_request_t* reqs, size_t n, int ndev, int32_t* route, int32_t* device,
                            uint32_t* tiles, uint32_t* slots) {
  if (ndev <= 0) return fail(P1HIP_ERR_ARGS, "ndev <= 0");
  if (n == 0) return P1HIP_OK;
  if (!reqs || !route || !device || !tiles || !slots) return fail(P1HIP_ERR_ARGS, "null request or output array");
  return guarded([&]() {
    if (int rc = below_batch_check(reqs, n)) return rc;
    Runtime& R = rt();
    std::lock_guard<std::mutex> g(R.mu);  // the split setting is the open devices'
    const bool split = R.devs.empty() ? !knob(kNoSplitKnob) : R.split;
    const int path = (int)knob(kBelowPathKnob);
    const uint64_t max_slice = knob(kBelowMaxSliceKnob);
    const std::vector<BelowBReq> q = below_batch_reqs(reqs, n);
    std::vector<int> routes;
    std::vector<size_t> live;
    std::vector<BelowWState> st;
    beloww_routes(q, path, max_slice, routes, live, st);
    for (size_t i = 0; i < n; ++i) {
      route[i] = routes[i];
      device[i] = -1;
      tiles[i] = slots[i] = 0;
    }
    std::vector<BelowBItem> dense;
    std::vector<BelowWItem> sparse;
    std::string err = beloww_round_items(q.data(), live, st, path, max_slice, dense, sparse);
    if (!err.empty()) return fail(P1HIP_ERR_HIP, err);
    for (const BelowBLaunch& L : belowb_layout(dense, ndev))
      for (size_t it : L.items) {
        const size_t i = live[dense[it].req];
        device[i] = L.device;
        tiles[i] = dense[it].tiles;
        slots[i] = dense[it].slots;
      }
    if (sparse.empty()) return P1HIP_OK;
    std::vector<size_t> pending(sparse.size());
    for (size_t s = 0; s < sparse.size(); ++s) pending[s] = s;
    BelowWGroup G;
    err = beloww_next_group(q.data(), live, sparse, pending, ndev, (uint32_t)knob(kWideMaxSegsKnob),
                            knob(kWideMinFastThreadsKnob), split, kWideMaxTiles, G);
    if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
    for (size_t m = 0; m < G.members.size(); ++m) {
      if (G.Y.route[m] != kWideRouteWide) continue;
      const BelowWItem& it = sparse[G.members[m]];
      const size_t i = live[it.req];
      device[i] = G.Y.device[m];
      tiles[i] = G.Y.tiles[m];
      slots[i] = beloww_slots(it.hi - it.lo + 1, q[i].target, G.Y.tiles[m], knob(kBelowWideMaxSlotsKnob));
    }
    return P1HIP_OK;
  });
}

int p1hip_get_below_wide_stats(p1hip_below_wide_stats_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null stats pointer");
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  *out = R.fstats;
  return P1HIP_OK;
}

int p1hip_below_filter(const uint64_t* part_hash, const uint64_t* part_nonce, size_t ntiles, const uint32_t* range_tile0,
                       const uint32_t* range_ntiles, const uint32_t* req_range0, const uint64_t* targets,
                       const uint32_t* req_slot0, size_t nreq, uint32_t* cand, uint32_t* count) {
  if (nreq == 0) return P1HIP_OK;
  if (!req_range0 || !req_slot0 || !targets || !count) return fail(P1HIP_ERR_ARGS, "null table, target or count array");
  if (nreq > kWideMaxTiles || ntiles > kWideMaxTiles) return fail(P1HIP_ERR_ARGS, "too many requests or tiles");
  // the kernel trusts its tables: every bound it relies on is checked here
  if (req_range0[0] != 0 || req_slot0[0] != 0) return fail(P1HIP_ERR_ARGS, "a request table does not start at 0");
  for (size_t r = 0; r < nreq; ++r)
    if (req_range0[r + 1] < req_range0[r] || req_slot0[r + 1] < req_slot0[r])
      return fail(P1HIP_ERR_ARGS, "request " + std::to_string(r) + ": a request table falls");
  if (req_range0[nreq] > kWideMaxTiles || req_slot0[nreq] > kWideMaxTiles)
    return fail(P1HIP_ERR_ARGS, "more than 2^24 ranges or slots");
  if (req_range0[nreq] > 0 && (!range_tile0 || !range_ntiles)) return fail(P1HIP_ERR_ARGS, "null range table");
  for (size_t j = 0; j < req_range0[nreq]; ++j)
    if (range_tile0[j] > ntiles || range_ntiles[j] > ntiles - range_tile0[j])
      return fail(P1HIP_ERR_ARGS, "range " + std::to_string(j) + " lies outside the partial array");
  if ((ntiles > 0 && (!part_hash || !part_nonce)) || (!cand && req_slot0[nreq] > 0))
    return fail(P1HIP_ERR_ARGS, "null partial or cand array");
  return guarded([&]() {
    return below_filter_locked(part_hash, part_nonce, ntiles, range_tile0, range_ntiles, req_range0, targets, req_slot0,
                               nreq, cand, count);
  });
}

int p1hip_scan_batch(const p1hip_request_t* reqs, size_t n, p1hip_result_t* out) {
  if (n == 0) return P1HIP_OK;
  if (!reqs || !out) return fail(P1HIP_ERR_ARGS, "null request or result array");
  return guarded([&]() {
    const int rc = batch_check(reqs, n);
    return rc ? rc : scan_batch_locked(reqs, n, out);
  });
}

int p1hip_batch_layout(const p1hip_request_t* reqs, size_t n, int ndev, uint32_t* tiles, int32_t* device,
                       int32_t* launch) {
  if (ndev <= 0) return fail(P1HIP_ERR_ARGS, "ndev <= 0");
  if (n == 0) return P1HIP_OK;
  if (!reqs || !tiles || !device || !launch) return fail(P1HIP_ERR_ARGS, "null request or output array");
  return guarded([&]() {
    const int rc = batch_check(reqs, n);
    if (rc) return rc;
    const std::vector<BatchReq> q = batch_reqs(reqs, n);
    const BatchLayout Y = batch_layout(q.data(), n, ndev, knob(kBatchMaxNoncesKnob), knob(kBatchMaxTilesKnob));
    for (size_t i = 0; i < n; ++i) {
      tiles[i] = Y.tiles[i];
      device[i] = Y.device[i];
      launch[i] = Y.launch[i];
    }
    return P1HIP_OK;
  });
}

int p1hip_get_batch_stats(p1hip_batch_stats_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null stats pointer");
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  *out = R.bstats;
  return P1HIP_OK;
}

int p1hip_scan_batch_wide(const p1hip_request_t* reqs, size_t n, p1hip_result_t* out) {
  if (n == 0) return P1HIP_OK;
  if (!reqs || !out) return fail(P1HIP_ERR_ARGS, "null request or result array");
  return guarded([&]() {
    const int rc = batch_check(reqs, n);
    return rc ? rc : scan_batch_wide_locked(reqs, n, out);
  });
}

int p1hip_wide_layout(const p1hip_request_t* reqs, size_t n, int ndev, int32_t* route, int32_t* device,
                      uint32_t* segs, uint32_t* tiles) {
  if (ndev <= 0) return fail(P1HIP_ERR_ARGS, "ndev <= 0");
  if (n == 0) return P1HIP_OK;
  if (!reqs || !route || !device || !segs || !tiles) return fail(P1HIP_ERR_ARGS, "null request or output array");
  return guarded([&]() {
    const int rc = batch_check(reqs, n);
    if (rc) return rc;
    Runtime& R = rt();
    std::lock_guard<std::mutex> g(R.mu);
    WideLayout Y;
    const std::string err = wide_layout_held(R, batch_reqs(reqs, n), ndev, Y);
    if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
    for (size_t i = 0; i < n; ++i) {
      route[i] = Y.route[i];
      device[i] = Y.device[i];
      segs[i] = Y.segs[i];
      tiles[i] = Y.tiles[i];
    }
    return P1HIP_OK;
  });
}

int p1hip_wide_ranges(const p1hip_request_t* reqs, size_t n, int ndev, size_t cap, size_t* count, uint32_t* req,
                      uint32_t* tile0, uint32_t* ntiles, int32_t* launch, uint32_t* dev_tiles) {
  if (ndev <= 0) return fail(P1HIP_ERR_ARGS, "ndev <= 0");
  if (!count || !dev_tiles || (cap && (!req || !tile0 || !ntiles || !launch)) || (n && !reqs))
    return fail(P1HIP_ERR_ARGS, "null request or output array");
  return guarded([&]() {
    const int rc = batch_check(reqs, n);
    if (rc) return rc;
    Runtime& R = rt();
    std::lock_guard<std::mutex> g(R.mu);
    WideLayout Y;
    const std::string err = wide_layout_held(R, batch_reqs(reqs, n), ndev, Y);
    if (!err.empty()) return fail(P1HIP_ERR_ARGS, err);
    size_t k = 0;
    for (int dv = 0; dv < ndev; ++dv) {
      const WideDevice& D = Y.devs[(size_t)dv];
      dev_tiles[dv] = D.total_tiles;
      for (size_t r = 0; r < D.reqs.size(); ++r)
        for (uint32_t j = D.req_range0[r]; j < D.req_range0[r + 1]; ++j, ++k) {
          if (k >= cap) continue;
          req[k] = (uint32_t)D.reqs[r];
          tile0[k] = D.ranges[j].tile0;
          ntiles[k] = D.ranges[j].ntiles;
          launch[k] = D.range_launch[j];
        }
    }
    *count = k;
    return P1HIP_OK;
  });
}

int p1hip_get_wide_stats(p1hip_wide_stats_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null stats pointer");
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  *out = R.wstats;
  return P1HIP_OK;
}

int p1hip_batch_submit(const p1hip_request_t* reqs, size_t n, int wide, p1hip_ticket_t* ticket) {
  if (!ticket) return fail(P1HIP_ERR_ARGS, "null ticket pointer");
  if (n && !reqs) return fail(P1HIP_ERR_ARGS, "null request array");
  return guarded([&]() {
    const int rc = batch_check(reqs, n);
    return rc ? rc : batch_submit_locked(reqs, n, wide != 0, ticket);
  });
}

int p1hip_batch_wait(p1hip_ticket_t ticket, p1hip_result_t* out) {
  return guarded([&]() { return batch_wait_locked(ticket, out); });
}

int p1hip_get_async_stats(p1hip_async_stats_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null stats pointer");
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  *out = R.astats;
  return P1HIP_OK;
}

int p1hip_plan_shards(const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper, int n,
                      uint64_t* first, uint64_t* last) {
  if (n <= 0 || !first || !last) return fail(P1HIP_ERR_ARGS, "n <= 0 or null output");
  if (!msg && msg_len > 0) return fail(P1HIP_ERR_ARGS, "msg == NULL with msg_len > 0");
  if (msg_len > P1HIP_MAX_MSG_LEN) return fail(P1HIP_ERR_ARGS, "msg_len exceeds P1HIP_MAX_MSG_LEN");
  if (lower > upper) {
    for (int i = 0; i < n; ++i) { first[i] = 1; last[i] = 0; }
    return P1HIP_OK;
  }
  return guarded([&]() {
    plan_shards(msg, msg_len, lower, upper, n, first, last);
    return P1HIP_OK;
  });
}

int p1hip_hash(const uint8_t* msg, size_t msg_len, uint64_t nonce, uint64_t* out_hash) {
  uint64_t n = 0;
  return p1hip_scan(msg, msg_len, nonce, nonce, out_hash, &n);
}

int p1hip_reduce_pairs(const uint64_t* hashes, const uint64_t* nonces, size_t n, uint64_t* out_hash,
                       uint64_t* out_nonce) {
  if (!out_hash || !out_nonce || (n && (!hashes || !nonces))) return fail(P1HIP_ERR_ARGS, "null pointer");
  return guarded([&]() { return reduce_pairs_locked(hashes, nonces, n, out_hash, out_nonce); });
}

int p1hip_set_profiling(int on) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  R.profiling = on != 0;
  return P1HIP_OK;
}

int p1hip_get_stats(p1hip_stats_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null stats pointer");
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  *out = R.stats;
  return P1HIP_OK;
}

void p1hip_reset_stats(void) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  R.stats = p1hip_stats_t{};
  R.bstats = p1hip_batch_stats_t{};
  R.wstats = p1hip_wide_stats_t{};
  R.astats = p1hip_async_stats_t{};
  R.lstats = p1hip_below_stats_t{};
  R.qstats = p1hip_below_batch_stats_t{};
  R.fstats = p1hip_below_wide_stats_t{};
  for (Dev& d : R.devs) {
    d.acc = p1hip_device_stats_t{};
    d.acc.shard_first = 1;  // empty until the next scan
  }
}

int p1hip_get_device_stats(int index, p1hip_device_stats_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null stats pointer");
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  if (index < 0 || (size_t)index >= R.devs.size()) return fail(P1HIP_ERR_ARGS, "device index out of range");
  *out = R.devs[(size_t)index].acc;
  out->ordinal = R.devs[(size_t)index].ordinal;
  return P1HIP_OK;
}

int p1hip_comm_info(int index, int* nranks, int* rank) {
  if (!nranks || !rank) return fail(P1HIP_ERR_ARGS, "null comm-info pointer");
  *nranks = 0;
  *rank = -1;
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  if (index < 0 || (size_t)index >= R.devs.size()) return fail(P1HIP_ERR_ARGS, "device index out of range");
  const Dev& d = R.devs[(size_t)index];
  if (!d.comm) return P1HIP_OK;  // one device without P1HIP_FORCE_RCCL, or host combine
  // what RCCL itself says, not what init asked for
  int count = 0, user = -1;
  NCCLCHK(ncclCommCount(d.comm, &count));
  NCCLCHK(ncclCommUserRank(d.comm, &user));
  *nranks = count;
  *rank = user;
  return P1HIP_OK;
}

int p1hip_abi_version(void) { return P1HIP_ABI_VERSION; }

const char* p1hip_last_error(void) { return g_err.c_str(); }

const char* p1hip_version(void) { return "p1hip 0.6 gfx950"; }

const char* p1hip_test_knobs(void) {
  static thread_local std::string s;
  s.clear();
  try {
    // the knobs the environment sets now (read per scan, or at the next init)
    std::vector<std::pair<std::string, std::string>> kv;
    if (test_knobs_on()) {
      kv.push_back({"P1HIP_TEST_KNOBS", "1"});
      for (const Knob& K : kKnobs)
        if (const char* v = test_knob(K.name)) kv.push_back({K.name, v});
    }
    // ... and the ones read at init that the open devices still run with,
    // even if the environment has changed since
    Runtime& R = rt();
    std::lock_guard<std::mutex> g(R.mu);
    auto add = [&](KnobId id, const std::string& v) {
      const char* k = kKnobs[id].name;
      for (auto& e : kv)
        if (e.first == k) {
          if (e.second != v) e.second += " (init: " + v + ")";
          return;
        }
      kv.push_back({k, "(init: " + v + ")"});
    };
    if (!R.devs.empty()) {
      if (R.min_fast_threads != kMinFastThreads) add(kMinFastThreadsKnob, std::to_string(R.min_fast_threads));
      if (R.fail_device >= 0) add(kTestFailDeviceKnob, std::to_string(R.fail_device));
      if (!R.tabulate) add(kNoTableKnob, "1");
      if (!R.split) add(kNoSplitKnob, "1");
      if (!R.use_rccl) add(kNoRcclKnob, "1");
      if (R.rccl_one) add(kForceRcclKnob, "1");
    }
    for (size_t i = 0; i < kv.size(); ++i) s += (i ? ";" : "") + kv[i].first + "=" + kv[i].second;
  } catch (...) {
    s = "?";  // never empty when the state could not be read
  }
  return s.c_str();
}

int p1hip_device_info(int index, p1hip_device_info_t* out) {
  if (!out) return fail(P1HIP_ERR_ARGS, "null info pointer");
  return guarded([&]() {
    Runtime& R = rt();
    std::lock_guard<std::mutex> g(R.mu);
    if (index < 0 || (size_t)index >= R.devs.size()) return fail(P1HIP_ERR_ARGS, "device index out of range");
    const int o = R.devs[(size_t)index].ordinal;
    memset(out, 0, sizeof *out);
    out->ordinal = o;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, o));
    HIPCHK(hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof out->pci_bus_id - 1, o));
    out->cu_count = prop.multiProcessorCount;
    out->clock_khz = prop.clockRate;
    out->hbm_bytes = (uint64_t)prop.totalGlobalMem;
    strncpy(out->arch, prop.gcnArchName, sizeof out->arch - 1);
    static_assert(sizeof(prop.uuid.bytes) == sizeof(out->uuid), "uuid size");
    memcpy(out->uuid, prop.uuid.bytes, sizeof out->uuid);
    return P1HIP_OK;
  });
}

void p1hip_shutdown(void) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> g(R.mu);
  shutdown_locked(R);
}

}  // extern "C"
