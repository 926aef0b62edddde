/*
 * p1hip.h -- C ABI of libp1hip.so, the MI355X (gfx950) drop-in for the
 * bitcoin miner's nonce scan.
 *
 * Reference seam (paths relative to /root/reference, SRC = src/github.com/cmu440):
 *   SRC/bitcoin/miner/miner.go:56-63   the loop this library replaces:
 *       var min, minIndex uint64 = math.MaxUint64, 0
 *       for i := req.Lower; i <= req.Upper; i++ {
 *           res := bitcoin.Hash(req.Data, i)
 *           if res < min { min = res; minIndex = i }
 *       }
 *   SRC/bitcoin/hash.go:13-17          bitcoin.Hash(msg, nonce) =
 *       BigEndian.Uint64(SHA-256(fmt.Sprintf("%s %d", msg, nonce))[0:8])
 *   SRC/bitcoin/message.go:18-44       Request{Data, Lower, Upper} in,
 *                                      Result{Hash, Nonce} out.
 * The reference has no FFI of its own; these are the entry points a cgo
 * bridge in the miner binds (INTEGRATION.md shows the binding).
 *
 * Plain C: no HIP/torch types, caller-owned buffers, no allocation crosses
 * the boundary.  `msg` is only borrowed for the duration of a call (cgo's
 * pointer-passing rule).  All calls are synchronous and serialised
 * internally, except the p1hip_batch_submit / p1hip_batch_wait pair below;
 * every call may be made from any host thread.
 *
 * Return codes: 0 ok; negative values are errors (details in
 * p1hip_last_error(), a per-thread string).
 */
#ifndef P1HIP_H
#define P1HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P1HIP_OK 0
#define P1HIP_ERR_NO_DEVICE (-1) /* no gfx950 device visible / bad ordinal      */
#define P1HIP_ERR_HIP (-2)       /* HIP runtime error, or a host-side failure
                                    (allocation, thread creation): no C++
                                    exception ever crosses this ABI            */
#define P1HIP_ERR_RCCL (-3)      /* RCCL error (multi-device all-gather)        */
#define P1HIP_ERR_ARGS (-4)      /* msg==NULL with msg_len>0, msg_len too large */

/* Longest message accepted (bytes).  Keeps the SHA-256 bit length in one
 * 32-bit word; the reference's LSP frames cap Data at ~1.3 KB anyway
 * (SRC/lsp/common.go:7, 2000-byte receive buffers). */
#define P1HIP_MAX_MSG_LEN ((size_t)1 << 28)

/* Open `want_devices` devices (<= 0: every visible device), create one HIP
 * stream per device and, when more than one device is used, one RCCL
 * communicator per device (ncclCommInitAll).  Idempotent: a second call with
 * the same count is a no-op; a different count re-initialises. */
int p1hip_init(int want_devices, int *got_devices);

/* Same, but with an explicit list of device ordinals (e.g. {LOCAL_RANK} for
 * a one-process-per-GPU miner). */
int p1hip_init_devices(const int *ordinals, int n);

/* The drop-in for miner.go:56-63.  Scans [lower, upper] INCLUSIVE and
 * returns the minimum bitcoin.Hash(msg, i) and its nonce; ties go to the
 * lowest nonce (strict '<' at miner.go:59).  lower > upper returns
 * (UINT64_MAX, 0) with rc 0, exactly like the reference loop.  If every hash
 * in the range equals UINT64_MAX the nonce is 0 (identity of miner.go:56).
 * Documented divergence: upper == UINT64_MAX is scanned inclusively and the
 * call returns; the Go loop wraps (i++) and never terminates.
 * With several devices the range is split contiguously across them
 * (p1hip_plan_shards) and the 16-byte per-device partials are combined by an
 * RCCL all-gather + host min.
 * Lazily calls p1hip_init(0, NULL) if nothing is initialised. */
int p1hip_scan(const uint8_t *msg, size_t msg_len, uint64_t lower, uint64_t upper,
               uint64_t *out_hash, uint64_t *out_nonce);

/* The contiguous split p1hip_scan uses across devices, for callers that
 * shard themselves (one process per GPU, or a server handing miners pieces
 * of one request, server.go:119-140): [lower, upper] (inclusive) into n >= 1
 * shards of near-equal predicted GPU time, in order; shard i is
 * [first[i], last[i]], and first[i] > last[i] marks an empty shard.  Host
 * only (no device needed).  Kernel variants differ in cost per nonce by
 * decade (digit count), so equal-count shards over different decades would
 * finish at different times.  Contiguous shards keep the lexicographic min
 * of the shard results equal to the serial first-minimum of miner.go:56-63.
 * lower > upper gives n empty shards. */
int p1hip_plan_shards(const uint8_t *msg, size_t msg_len, uint64_t lower, uint64_t upper, int n,
                      uint64_t *first, uint64_t *last);

/* bitcoin.Hash(msg, nonce) (hash.go:13-17), computed on the GPU as the
 * one-nonce scan [nonce, nonce]. */
int p1hip_hash(const uint8_t *msg, size_t msg_len, uint64_t nonce, uint64_t *out_hash);

/* Test hook for the device-side argmin: reduces n crafted (hash, nonce)
 * pairs with the scan's own wave/LDS/grid reduction kernels and applies the
 * same result rules as p1hip_scan (lexicographic (hash, nonce) minimum,
 * nonce 0 when the minimum hash is UINT64_MAX, (UINT64_MAX, 0) when n == 0). */
int p1hip_reduce_pairs(const uint64_t *hashes, const uint64_t *nonces, size_t n,
                       uint64_t *out_hash, uint64_t *out_nonce);

/* Test hook like p1hip_reduce_pairs, for the per-tile witness of
 * tests/test_gpu_tiles.py: one scan of [lower, upper] (1 .. 2^32 nonces; an
 * empty or larger range is P1HIP_ERR_ARGS) on the first open device, through
 * the very code p1hip_scan runs for a share of that size (k_scan launches +
 * k_reduce, or k_scan_small for at most 2^16 nonces; same planner settings,
 * tables, packing and test knobs), with two additions: the scan's slice of
 * the partial array is filled with the byte P1HIP_TILE_POISON first (on the
 * device's own stream), and every workgroup partial is copied back raw.
 * tiles[i] is entry i of the partial array: the launch and tile that wrote
 * it, its segment's kind (variant id, 255 = generic) and k, the tile's exact
 * nonce set -- `nruns` <= 4 strided runs: run r covers, for j in [0, count),
 * the run_len consecutive nonces from first + j * stride; nruns == 0 is a
 * tile without a valid thread, whose partial is (UINT64_MAX, UINT64_MAX) --
 * and the (hash, nonce) found there.  The map is that of the plan and packing
 * actually launched.  *count receives the number of tiles; only the first
 * `cap` entries are written.  *route: 0 = k_scan, 1 = k_scan_small.
 * *out_hash / *out_nonce: the finished result, as p1hip_scan returns it.
 * Counts in no statistics. */
#define P1HIP_TILE_POISON 0xA5
typedef struct { uint64_t first, stride; uint32_t run_len, count; } p1hip_tile_run_t;
typedef struct {
  uint32_t launch, tile, kind, k, nruns, reserved;
  p1hip_tile_run_t runs[4];
  uint64_t hash, nonce;
} p1hip_tile_t;
int p1hip_scan_tiles(const uint8_t *msg, size_t msg_len, uint64_t lower, uint64_t upper, size_t cap,
                     size_t *count, p1hip_tile_t *tiles, int *route, uint64_t *out_hash, uint64_t *out_nonce);

/* Many requests in one call.  A miner that serves many clients' small jobs,
 * or a chunk loop over short ranges, is bound by launch and completion
 * latency when it calls p1hip_scan once per request: a configs[0]-sized
 * request fills a few percent of the device.  p1hip_scan_batch coalesces
 * every non-empty request of at most 2^16 nonces -- of any messages -- into
 * one launch pair per device (k_batch_scan: one workgroup per 256 nonces of
 * any request; k_batch_reduce: one workgroup per request), with one stream
 * synchronisation per launch pair; a launch pair holds up to 2^20 workgroups.
 * Larger requests run one by one through the p1hip_scan path, empty ranges
 * are answered on the host. */
typedef struct { const uint8_t *msg; size_t msg_len; uint64_t lower, upper; } p1hip_request_t;
typedef struct { uint64_t hash, nonce; } p1hip_result_t;

/* out[i] is exactly what p1hip_scan(reqs[i]...) would return, for every i.
 * Every request is validated (as by p1hip_scan) before anything is launched:
 * a bad one gives P1HIP_ERR_ARGS, p1hip_last_error() names its index and
 * `out` is left untouched, as it is after any other error.  n == 0 returns 0
 * without initialising a device; otherwise lazy init as in p1hip_scan.  With
 * several devices the coalesced requests are cut into contiguous groups of
 * near-equal workgroup count, one per device (no RCCL: a request lives wholly
 * on one device), all launched before any stream is synchronised. */
int p1hip_scan_batch(const p1hip_request_t *reqs, size_t n, p1hip_result_t *out);

/* Host only (no device): how a batch would be laid out over ndev devices.
 * tiles[i]: workgroup tiles of request i (0: empty range, or run individually);
 * device[i] / launch[i]: the device (index as for p1hip_get_device_stats) and
 * that device's launch pair (from 0) its coalesced launch goes to (-1: empty
 * or individual).  p1hip_scan_batch lays its requests out with the same
 * function. */
int p1hip_batch_layout(const p1hip_request_t *reqs, size_t n, int ndev,
                       uint32_t *tiles, int32_t *device, int32_t *launch);

/* Accounting of p1hip_scan_batch since p1hip_reset_stats.  Requests run
 * individually also count in p1hip_stats_t as scans; coalesced ones only here. */
typedef struct {
  uint64_t calls;            /* p1hip_scan_batch calls that succeeded             */
  uint64_t requests;         /* requests in them                                  */
  uint64_t coalesced;        /* ... answered by a coalesced launch pair           */
  uint64_t individual;       /* ... run one by one (more than 2^16 nonces)        */
  uint64_t empty;            /* ... with lower > upper (answered on the host)     */
  uint64_t launches;         /* launch pairs (k_batch_scan + k_batch_reduce)      */
  uint64_t tiles;            /* workgroups of k_batch_scan                        */
  uint64_t nonces;           /* nonces they hashed                                */
  double wall_ms;            /* host wall time inside p1hip_scan_batch            */
} p1hip_batch_stats_t;
int p1hip_get_batch_stats(p1hip_batch_stats_t *out);   /* cleared by p1hip_reset_stats */

/* Many requests in one call, mid-size ones included.  p1hip_scan_batch runs
 * every request above 2^16 nonces alone, but a job of 10^5..10^7 nonces (the
 * reference's own job size) is a handful of k_scan segments and a few dozen
 * workgroups on a device that holds about a thousand.  Here the requests
 * above 2^16 and of at most 2^24 nonces -- of any messages -- share k_scan
 * launches, up to 64 segments each; their ragged edges share one k_batch_scan
 * launch; k_wide_reduce folds one result per request; one copy back and one
 * stream synchronisation per device end the call.  Each request takes one
 * route (p1hip_wide_layout reports it):
 *   0 empty range (answered on the host)
 *   1 small: at most 2^16 nonces, p1hip_scan_batch's coalesced launch pair
 *   2 wide:  above that and at most 2^24 nonces, shared k_scan launches
 *   3 individual: larger, one by one through the p1hip_scan path
 * The contract is p1hip_scan_batch's: out[i] is exactly what
 * p1hip_scan(reqs[i]...) returns; every request is validated before anything
 * runs (P1HIP_ERR_ARGS names the index) and `out` is untouched on any error;
 * n == 0 returns 0 without opening a device.  With several devices the wide
 * requests are cut, in request order, into contiguous groups of near-equal
 * predicted cost, one per device (a request lives wholly on one device), all
 * enqueued before any stream is synchronised. */
int p1hip_scan_batch_wide(const p1hip_request_t *reqs, size_t n, p1hip_result_t *out);

/* Host only (no device): how p1hip_scan_batch_wide would lay the call out
 * over ndev devices.  route[i]: as above; device[i]: the device of a wide
 * request (-1 otherwise); segs[i]: the k_scan segments of a wide request (its
 * fast pieces) and tiles[i]: all its workgroup tiles (both 0 otherwise).  A
 * wide request is planned with an occupancy floor of 2^18 / min(wide requests
 * on its device, 64) threads, so the more requests share the launches, the
 * more nonces each thread runs (10^k, k = 1..3) and the fewer tiles a request
 * has: tiles[i] shows the k chosen. */
int p1hip_wide_layout(const p1hip_request_t *reqs, size_t n, int ndev,
                      int32_t *route, int32_t *device, uint32_t *segs, uint32_t *tiles);

/* Host only: the range table of the same layout, for tests and tools.  A
 * range is a run of tiles of one request in its device's partial array:
 * tiles [tile0[j], tile0[j] + ntiles[j]) of request req[j], written by k_scan
 * launch launch[j] of that device (from 0; -1: the device's k_batch_scan
 * launch of the generic pieces).  Ranges are listed by device, then request.
 * *count receives the number of ranges; only the first `cap` are written.
 * dev_tiles[d] (ndev entries) is the size of device d's partial array. */
int p1hip_wide_ranges(const p1hip_request_t *reqs, size_t n, int ndev, size_t cap, size_t *count,
                      uint32_t *req, uint32_t *tile0, uint32_t *ntiles, int32_t *launch,
                      uint32_t *dev_tiles);

/* Accounting of p1hip_scan_batch_wide since p1hip_reset_stats.  Its small
 * requests also count, as one p1hip_scan_batch call, in p1hip_batch_stats_t,
 * its individual ones in p1hip_stats_t as scans; wide ones only here. */
typedef struct {
  uint64_t calls;            /* p1hip_scan_batch_wide calls that succeeded        */
  uint64_t requests;         /* requests in them                                  */
  uint64_t empty;            /* ... per route: lower > upper                      */
  uint64_t small;            /*     at most 2^16 nonces                           */
  uint64_t wide;             /*     sharing k_scan launches                       */
  uint64_t individual;       /*     run one by one                                */
  uint64_t scan_launches;    /* k_scan launches of the wide route                 */
  uint64_t scan_segments;    /* segments in their tables (fast pieces)            */
  uint64_t generic_launches; /* k_batch_scan launches of the wide route           */
  uint64_t generic_segments; /* generic pieces in their tables                    */
  uint64_t tiles;            /* workgroup tiles of the wide route                 */
  uint64_t nonces;           /* nonces they hashed                                */
  double wall_ms;            /* host wall time inside p1hip_scan_batch_wide       */
} p1hip_wide_stats_t;
int p1hip_get_wide_stats(p1hip_wide_stats_t *out);     /* cleared by p1hip_reset_stats */

/* Asynchronous batches.  The calls above return when the device is done, so a
 * caller that marshals the next call, or writes the last one's results, does
 * so while the device idles.  p1hip_batch_submit lays a call out, copies what
 * it needs, enqueues it and returns WITHOUT synchronising; p1hip_batch_wait
 * blocks until that call is done and hands the results over.  Up to
 * P1HIP_MAX_INFLIGHT tickets may be outstanding, so the device runs call k
 * while the host prepares call k + 1 (one goroutine submits,
 * another waits).
 *
 * p1hip_batch_submit(reqs, n, wide, &ticket): the call p1hip_scan_batch
 * (wide == 0) or p1hip_scan_batch_wide (wide != 0) would make of the same
 * requests -- the same routes, layout, tables and launches
 * (p1hip_batch_layout / p1hip_wide_layout describe them), on each device's own
 * stream, followed by one event per device.  Every request is validated first
 * as the synchronous calls do (P1HIP_ERR_ARGS names the index).  `reqs` and
 * every `msg` are borrowed only until submit returns.  n == 0 gives a ticket
 * without opening a device (its wait returns 0); otherwise lazy init as in
 * p1hip_scan.  With P1HIP_MAX_INFLIGHT tickets outstanding the call returns
 * P1HIP_ERR_BUSY and enqueues nothing.  If anything fails after the first
 * enqueue the streams are drained, no ticket is issued and the error is
 * returned here.  *ticket is written only on success and is never 0.
 *
 * Requests on the individual route (more than 2^16 nonces with wide == 0,
 * more than 2^24 with wide != 0) are NOT enqueued by submit: they need the
 * MODE 5 tables and, with several devices, the all-gather of the p1hip_scan
 * path, which is synchronous.  p1hip_batch_wait runs them one by one through
 * that path once the ticket's coalesced part is done; a caller that wants
 * overlap keeps its requests at or below the limit (the pool's --chunk).
 *
 * p1hip_batch_wait(ticket, out): blocks on the ticket's events -- not holding
 * the library's lock, so other threads submit, wait and scan meanwhile --
 * then out[i] is exactly what p1hip_scan(reqs[i]...) returns, for every i.
 * `out` is written only on success; the ticket is spent and its slot free
 * again on success and on error alike.  Tickets may be waited in any order
 * and from any thread.  A ticket that is unknown, already waited (or being
 * waited by another thread), or cancelled gives P1HIP_ERR_ARGS.
 * p1hip_shutdown and a re-initialising p1hip_init* drain the streams and
 * cancel every outstanding ticket.
 *
 * Each of the P1HIP_MAX_INFLIGHT slots owns every buffer its call writes
 * (staging tables, device tables, partials, results), so a later submit never
 * rewrites what an earlier ticket still reads; the synchronous calls keep
 * their own buffers and stay legal while tickets are outstanding: they queue
 * behind them on the stream.  A ticket's requests count in
 * p1hip_batch_stats_t / p1hip_wide_stats_t as the synchronous call's would,
 * when its wait succeeds (wall_ms: the time inside submit plus inside wait). */
#define P1HIP_ERR_BUSY (-5)          /* P1HIP_MAX_INFLIGHT tickets are outstanding */
#define P1HIP_MAX_INFLIGHT 4
typedef uint64_t p1hip_ticket_t;     /* never 0 for a live ticket */
int p1hip_batch_submit(const p1hip_request_t *reqs, size_t n, int wide, p1hip_ticket_t *ticket);
int p1hip_batch_wait(p1hip_ticket_t ticket, p1hip_result_t *out);

/* Accounting of the two calls above since p1hip_reset_stats. */
typedef struct {
  uint64_t submits;          /* p1hip_batch_submit calls that issued a ticket     */
  uint64_t waits;            /* p1hip_batch_wait calls that succeeded             */
  uint64_t busy;             /* submits refused with P1HIP_ERR_BUSY               */
  uint64_t max_inflight;     /* most tickets outstanding at once                  */
  double submit_ms;          /* host wall time inside successful submits          */
  double wait_ms;            /* ... inside successful waits (blocking included)   */
} p1hip_async_stats_t;
int p1hip_get_async_stats(p1hip_async_stats_t *out);   /* cleared by p1hip_reset_stats */

/* Every nonce whose hash is at or below a target.  The calls above answer
 * "the minimum over a range"; a miner is normally asked the other question:
 *     for i := lower; i <= upper; i++ { if bitcoin.Hash(data, i) <= target { hits = append(hits, i) } }
 * With cap == 1 that is "the first nonce that meets the target", with a larger
 * cap "every share in the range".
 *
 * hits = the nonces n of [lower, upper] (inclusive) with bitcoin.Hash(msg, n)
 * <= target, in increasing n, the first `cap` of them; hits[i] = {hash, nonce}.
 * *found < cap: these are ALL hits of the range.  *found == cap: there may be
 * more; resume with lower = hits[cap-1].nonce + 1.
 * The comparison is <=: target 0 asks for a hash equal to 0, UINT64_MAX for
 * every nonce.  lower > upper or cap == 0 gives *found = 0 with rc 0 and opens
 * no device.  upper == UINT64_MAX is scanned inclusively.  Arguments are
 * validated as p1hip_scan validates them; `hits` and `found` are written only
 * on success.  Synchronous, serialised under the library's lock, lazy init as
 * in p1hip_scan; legal while tickets are outstanding (it owns every buffer it
 * adds, and shares p1hip_scan's otherwise).  The result is defined by the loop
 * above alone: slicing, route and device count never show in it.
 *
 * The range is scanned in consecutive slices and the call returns after the
 * first slice that brings the total to `cap`.  A slice is twice the nonces
 * expected to hold the missing hits, 2 * want * 2^64 / (target + 1), rounded
 * up to a power of two and clamped to [2^16, P1HIP_BELOW_MAX_SLICE].  A slice
 * takes one of two routes, chosen from the target:
 *   sparse (target < P1HIP_BELOW_DENSE_TARGET): the slice is scanned exactly
 *     as p1hip_scan scans it (same plan, tables, packing, devices); k_scan's
 *     16-byte partial per tile, the tile's minimum, is the filter: only tiles
 *     whose partial is at or below the target are looked at nonce by nonce, by
 *     k_below_mark (one bit per nonce) on the first device.
 *   dense (otherwise, at most P1HIP_BELOW_MAX_SLICE_DENSE nonces a slice; and
 *     any slice of at most 2^16 nonces): every nonce goes straight to
 *     k_below_mark.
 * Two checks stay in the product, a failure of either is P1HIP_ERR_HIP: every
 * marked nonce's hash, recomputed on the host, is at or below the target; and
 * the marks of every refined tile have exactly the tile's partial (hash,
 * nonce) as their lexicographic minimum. */
#define P1HIP_BELOW_MAX_SLICE ((uint64_t)1 << 34)
#define P1HIP_BELOW_MAX_SLICE_DENSE ((uint64_t)1 << 28)
#define P1HIP_BELOW_DENSE_TARGET ((uint64_t)1 << 46)
int p1hip_scan_below(const uint8_t *msg, size_t msg_len, uint64_t lower, uint64_t upper,
                     uint64_t target, size_t cap, p1hip_result_t *hits, size_t *found);

/* Accounting of p1hip_scan_below since p1hip_reset_stats.  Its k_scan launches
 * also count in the p1hip_device_stats_t of the device that ran them, as
 * scan_launches, scan_nonces, scan_alg_ops and scan_kernel_ms; nothing of it
 * counts in p1hip_stats_t. */
typedef struct {
  uint64_t calls;            /* p1hip_scan_below calls that succeeded             */
  uint64_t slices;           /* slices they ran                                   */
  uint64_t sparse_slices;    /* ... filtered by k_scan                            */
  uint64_t dense_slices;     /* ... marked nonce by nonce                         */
  uint64_t examined;         /* nonces of the finished slices                     */
  uint64_t scan_nonces;      /* nonces hashed by k_scan (sparse slices)           */
  uint64_t mark_nonces;      /* nonces hashed by k_below_mark                     */
  uint64_t candidate_tiles;  /* k_scan tiles whose partial was <= target          */
  uint64_t mark_launches;    /* k_below_mark launches                             */
  uint64_t hits;             /* hits returned                                     */
  double wall_ms;            /* host wall time inside p1hip_scan_below            */
} p1hip_below_stats_t;
int p1hip_get_below_stats(p1hip_below_stats_t *out);   /* cleared by p1hip_reset_stats */

/* Many target searches in one call.  A pool that hands each worker its own
 * message and an easy share target asks p1hip_scan_below's question for
 * hundreds of messages at once, and each answer is a slice of 2^16..2^20
 * nonces: launch and completion latency on a device that holds about a
 * thousand workgroups.  Here the current slices of all such requests share one
 * launch pair per device: k_belowb_mark marks every nonce against its own
 * request's target and k_belowb_collect, one workgroup per request, turns the
 * marks into the indices of the request's first hits on the device, so a round
 * copies back 4 bytes per hit slot instead of one bit per nonce.
 *
 * Request i owns hits[off_i .. off_i + cap_i), off_i = the sum of the caps
 * before it; found[i] entries of that region are written and they are exactly
 * what p1hip_scan_below(reqs[i]..., cap_i, ...) returns: the hits of the
 * reference loop in increasing nonce, the first cap_i of them, with the same
 * found < cap / found == cap meaning.  The result is defined by that loop
 * alone: rounds, routes, launch pairs and device count never show in it.
 * The sum of the caps (computed with an overflow check) must be at most
 * hits_len, otherwise P1HIP_ERR_ARGS.  Every request is validated as
 * p1hip_scan_below validates it, before anything runs (P1HIP_ERR_ARGS names
 * the index); `hits` and `found` are untouched on any error.  n == 0, and a
 * call whose requests are all empty (lower > upper or cap == 0), opens no
 * device; otherwise lazy init as in p1hip_scan.  Synchronous, serialised under
 * the library's lock as p1hip_scan_below is; legal while tickets are
 * outstanding (it owns every buffer it adds, each device's own stream).
 *
 * Each request takes one route, fixed from its first slice (the slice rule and
 * its dense / sparse choice are p1hip_scan_below's; p1hip_below_batch_layout
 * reports the route):
 *   0 empty: lower > upper or cap == 0 (found[i] = 0)
 *   1 coalesced: the first slice is dense and has at most
 *     P1HIP_BELOW_BATCH_MAX_NONCES nonces.  That admits every cap = 1 request
 *     at a dense target (2 * 2^64 / 2^46 = 2^19) and cap = 2 at the switch
 *     target.  Later slices are never longer and stay dense.
 *   2 individual: every other request, one by one through p1hip_scan_below's
 *     own path after the coalesced part; these count in p1hip_below_stats_t as
 *     calls.
 * The coalesced requests advance in rounds.  A round takes the next slice of
 * every unfinished request, lays the slices out over the open devices as
 * p1hip_scan_batch lays its requests out (contiguous groups by tile count, a
 * request wholly on one device) and cuts a device's group into launch pairs
 * that close at 2^20 tiles or at P1HIP_BELOW_BATCH_MAX_SLOTS hit slots (a
 * request's slots in a round: min(hits still wanted, nonces of the slice)).
 * Every device is enqueued before any is synchronised: one copy back and one
 * stream synchronisation per device per round.  A request is finished when
 * found == cap or its slice ended at upper.
 * Checks kept in the product, a failure of any is P1HIP_ERR_HIP: every
 * returned index is a thread of its piece; its hash, recomputed on the host,
 * is at or below the request's target; a request's nonces are strictly
 * increasing; no request reports more hits than it has slots. */
#define P1HIP_BELOW_BATCH_MAX_NONCES ((uint64_t)1 << 20)
#define P1HIP_BELOW_BATCH_MAX_SLOTS ((uint64_t)1 << 22)
typedef struct {
  const uint8_t *msg;
  size_t msg_len;
  uint64_t lower, upper, target;
  size_t cap;
} p1hip_below_request_t;
int p1hip_scan_below_batch(const p1hip_below_request_t *reqs, size_t n,
                           p1hip_result_t *hits, size_t hits_len, size_t *found /* n */);

/* Host only (no device): the routes of a call and the layout of its first
 * round over ndev devices.  route[i]: as above; device[i]: the device of a
 * coalesced request's first slice (-1 otherwise); tiles[i]: that slice's
 * workgroup tiles (0 otherwise). */
int p1hip_below_batch_layout(const p1hip_below_request_t *reqs, size_t n, int ndev,
                             int32_t *route, int32_t *device, uint32_t *tiles);

/* Accounting of p1hip_scan_below_batch since p1hip_reset_stats.  Individual
 * requests also count in p1hip_below_stats_t as calls; coalesced ones only
 * here. */
typedef struct {
  uint64_t calls;            /* p1hip_scan_below_batch calls that succeeded       */
  uint64_t requests;         /* requests in them                                  */
  uint64_t empty;            /* ... per route: lower > upper or cap == 0          */
  uint64_t coalesced;        /*     sharing launch pairs                          */
  uint64_t individual;       /*     run one by one                                */
  uint64_t rounds;           /* rounds of the coalesced route                     */
  uint64_t launches;         /* launch pairs (k_belowb_mark + k_belowb_collect)   */
  uint64_t tiles;            /* workgroups of k_belowb_mark                       */
  uint64_t mark_nonces;      /* nonces they hashed                                */
  uint64_t hits;             /* hits returned (all routes)                        */
  uint64_t bytes_back;       /* bytes copied back from the devices (coalesced)    */
  double wall_ms;            /* host wall time inside p1hip_scan_below_batch      */
} p1hip_below_batch_stats_t;
int p1hip_get_below_batch_stats(p1hip_below_batch_stats_t *out);   /* cleared by p1hip_reset_stats */

/* Test hook: k_belowb_collect alone, on the first device, over crafted mark
 * words.  Request r of nreq owns words [4 * req_tile0[r], 4 * req_tile0[r + 1])
 * of `words` and slots [req_hit0[r], req_hit0[r + 1]) of `idx` (both tables
 * have nreq + 1 entries, start at 0 and never fall; at most 2^20 tiles and
 * P1HIP_BELOW_BATCH_MAX_SLOTS slots).  idx receives, per request, the thread
 * indices (64 * word + bit) of its first set bits in word and bit order, as
 * many as it has slots; count[r] their number; slots the kernel does not
 * write read UINT32_MAX.  Counts in no statistics. */
int p1hip_below_collect(const uint64_t *words, const uint32_t *req_tile0, const uint32_t *req_hit0,
                        size_t nreq, uint32_t *idx, uint32_t *count);

/* Hard-target searches share k_scan.  p1hip_scan_below_batch coalesces only
 * requests whose first slice is dense; a request with a hard target -- a pool's
 * share target, a server's "first nonce at or below T" over a chunk of 2^24
 * nonces -- has a sparse first slice of 2^16..2^24 nonces and would run alone:
 * a k_scan launch of a few dozen workgroups, a copy back of every partial, a
 * host filter, a mark launch, two synchronisations.  Here the sparse slices of
 * all such requests share k_scan launches exactly as the wide requests of
 * p1hip_scan_batch_wide do, k_beloww_filter (a fifth code object) turns each
 * request's partials into its candidate tiles on the device, and one
 * k_belowb_mark launch per device refines all candidates of all its requests.
 *
 * The contract is p1hip_scan_below_batch's, word for word: request i owns
 * hits[off_i .. off_i + cap_i), off_i = the sum of the caps before it (computed
 * with an overflow check; above hits_len: P1HIP_ERR_ARGS); found[i] entries of
 * it are written and they are exactly what p1hip_scan_below(reqs[i]...)
 * returns; every request is validated before anything runs (P1HIP_ERR_ARGS
 * names the index); `hits` and `found` are untouched on any error; n == 0 and
 * a call whose requests are all empty open no device; synchronous under the
 * library's lock; legal while tickets are outstanding.  Routes, rounds, groups
 * and device count never show in the result.
 *
 * Routes, fixed from the first slice (p1hip_below_wide_layout reports them):
 *   0 empty: lower > upper or cap == 0
 *   1 coalesced: the first slice is dense and has at most
 *     P1HIP_BELOW_BATCH_MAX_NONCES nonces: p1hip_scan_below_batch's route and
 *     machinery
 *   3 filtered: the first slice is sparse and has at most
 *     P1HIP_BELOW_WIDE_MAX_NONCES nonces
 *   2 individual: every other request, one by one through p1hip_scan_below's
 *     own path after the rounds; these count in p1hip_below_stats_t as calls
 * A later slice is never longer than the first; a filtered request's later
 * slice is sparse, or has fallen to at most 2^16 nonces and become dense, and
 * then it goes through the dense launch pair of the same round; a coalesced
 * request never turns sparse.
 *
 * A round takes the next slice of every unfinished coalesced and filtered
 * request.  The dense slices go into launch pairs as in p1hip_scan_below_batch.
 * The sparse ones run in groups (one, unless a device's partial array of 2^24
 * tiles is full: the slices turned away form a further group of the round).
 * Phase A of a group, every device enqueued before any is synchronised: the
 * shared k_scan launches, one k_batch_scan for the ragged edges, then
 * k_beloww_filter, one workgroup per request, which writes the indices of the
 * request's first `slots` candidate tiles (partial at or below the target) and
 * the number of all of them; one count per request and its slots are copied
 * back.  slots = min(tiles, 16 + 4 * ceil(len * (target + 1) / 2^64)): four
 * times the expected hits of the slice plus 16.  A request that reports more
 * candidates than slots is still answered exactly: the host copies that
 * request's partials back and filters them itself (slot_overflows).  Phase B:
 * the host turns every candidate into its tile's nonces, k_belowb_mark marks
 * them on the request's own device against the request's own target, and the
 * marks are copied back and decoded.
 * Checks kept in the product, a failure of any is P1HIP_ERR_HIP: every
 * candidate index lies in its request's ranges, in table order; its partial is
 * at or below the target; every marked thread is a nonce of its piece and its
 * hash, recomputed on the host, is at or below the target; each candidate
 * tile's refinement has exactly the tile's partial as its minimum; a request's
 * nonces are strictly increasing across rounds; and p1hip_scan_below_batch's
 * own checks for the dense slices. */
#define P1HIP_BELOW_WIDE_MAX_NONCES ((uint64_t)1 << 24)
int p1hip_scan_below_batch_wide(const p1hip_below_request_t *reqs, size_t n,
                                p1hip_result_t *hits, size_t hits_len, size_t *found /* n */);

/* Host only (no device): the routes of a call and the layout of its first
 * round (first group) over ndev devices.  route[i]: as above; device[i]: the
 * device of a coalesced or filtered request's first slice (-1 otherwise; -1
 * also for a filtered slice deferred to a further group); tiles[i]: that
 * slice's workgroup tiles (0 otherwise); slots[i]: a coalesced slice's hit
 * slots, a filtered slice's candidate slots (0 otherwise). */
int p1hip_below_wide_layout(const p1hip_below_request_t *reqs, size_t n, int ndev,
                            int32_t *route, int32_t *device, uint32_t *tiles, uint32_t *slots);

/* Accounting of p1hip_scan_below_batch_wide since p1hip_reset_stats.
 * Individual requests also count in p1hip_below_stats_t as calls; the k_scan
 * launches also count in each device's p1hip_device_stats_t.
 * p1hip_below_batch_stats_t is not touched. */
typedef struct {
  uint64_t calls;            /* p1hip_scan_below_batch_wide calls that succeeded  */
  uint64_t requests;         /* requests in them                                  */
  uint64_t empty;            /* ... per route: lower > upper or cap == 0          */
  uint64_t coalesced;        /*     dense, sharing launch pairs                   */
  uint64_t filtered;         /*     sparse, sharing k_scan launches               */
  uint64_t individual;       /*     run one by one                                */
  uint64_t rounds;           /* rounds of the coalesced and filtered routes       */
  uint64_t groups;           /* groups of sparse slices (wide_layout calls)       */
  uint64_t scan_launches;    /* shared k_scan launches                            */
  uint64_t scan_segments;    /* segments in them                                  */
  uint64_t generic_launches; /* k_batch_scan launches (ragged edges)              */
  uint64_t scan_nonces;      /* nonces of the sparse slices (both kernels)        */
  uint64_t filter_launches;  /* k_beloww_filter launches                          */
  uint64_t candidate_tiles;  /* tiles with a partial <= target and a valid thread */
  uint64_t slot_overflows;   /* requests of a round with more candidates than
                                slots, answered by the host filter               */
  uint64_t mark_launches;    /* k_belowb_mark launches (dense pairs and phase B)  */
  uint64_t mark_tiles;       /* workgroups of those launches                      */
  uint64_t mark_nonces;      /* nonces they hashed                                */
  uint64_t hits;             /* hits returned (all routes)                        */
  uint64_t bytes_back;       /* bytes copied back from the devices (rounds)       */
  double wall_ms;            /* host wall time inside the call                    */
} p1hip_below_wide_stats_t;
int p1hip_get_below_wide_stats(p1hip_below_wide_stats_t *out);   /* cleared by p1hip_reset_stats */

/* Test hook: k_beloww_filter alone, on the first device, over a crafted partial
 * array of ntiles (hash, nonce) pairs.  Request r of nreq owns the ranges
 * [range_tile0[j], range_tile0[j] + range_ntiles[j]) for j in
 * [req_range0[r], req_range0[r + 1]) and slots [req_slot0[r], req_slot0[r + 1])
 * of `cand` (both request tables have nreq + 1 entries, start at 0 and never
 * fall; every range lies inside the array; at most 2^24 tiles, 2^24 slots and
 * 2^24 ranges).  cand receives, per request, the partial-array indices of its
 * first tiles with hash <= targets[r], in table order, as many as it has
 * slots; count[r] the number of all such tiles, not clamped; slots the kernel
 * does not write read UINT32_MAX.  Counts in no statistics. */
int p1hip_below_filter(const uint64_t *part_hash, const uint64_t *part_nonce, size_t ntiles,
                       const uint32_t *range_tile0, const uint32_t *range_ntiles,
                       const uint32_t *req_range0, const uint64_t *targets, const uint32_t *req_slot0,
                       size_t nreq, uint32_t *cand, uint32_t *count);

/* Kernel-level accounting.  One p1hip_scan = one (rarely several) launch of
 * the scan kernel k_scan per device, covering every decade of the range; a
 * share of at most 2^16 nonces is one launch of k_scan_small instead (plan in
 * the kernel arguments, reduce fused into the last workgroup, result written
 * to pinned host memory). */
typedef struct {
  uint64_t scans;            /* p1hip_scan calls since reset                      */
  uint64_t fast_launches;    /* fast segments (one thread per 10^k nonces)        */
  uint64_t fast_nonces;      /* nonces hashed by fast segments                    */
  uint64_t fast_alg_ops;     /* algorithmic int32 ops: 1384 * B_tail per nonce    */
  uint64_t generic_launches; /* generic segments (one thread per nonce)           */
  uint64_t generic_nonces;   /* nonces hashed by generic segments                 */
  double scan_wall_ms;       /* host wall time inside p1hip_scan                  */
  uint64_t scan_launches;    /* launches of k_scan                                */
  uint64_t scan_nonces;      /* nonces hashed by those launches                   */
  uint64_t scan_alg_ops;     /* their algorithmic int32 ops (1384 * B_tail each)  */
  double scan_kernel_ms;     /* sum of HIP-event durations of those launches
                                (recorded only while profiling is on)            */
  uint64_t small_scans;      /* device scans that took the one-launch small path
                                (<= 2^16 nonces: k_scan_small, fused reduce)     */
  uint64_t table_replans;    /* device shares re-planned without MODE 5 because a
                                K+W table could not be had (before any launch)   */
} p1hip_stats_t;

/* Per-device accounting since p1hip_reset_stats (device `index` in the order
 * p1hip_init / p1hip_init_devices opened them), so a multi-device scan can
 * explain its own scaling: which shard each device took, how long its
 * kernels ran, how long its host thread spent in the scan phase and in the
 * all-gather phase. */
typedef struct {
  int32_t ordinal;           /* HIP device ordinal                                */
  int32_t active;            /* its shard of the last scan was non-empty          */
  uint64_t shard_first;      /* last scan's shard [first, last] (first > last:    */
  uint64_t shard_last;       /*   empty)                                          */
  uint64_t scans;            /* p1hip_scan calls this device took part in         */
  uint64_t scan_launches;    /* k_scan / k_scan_small launches                    */
  uint64_t scan_nonces;      /* nonces they hashed                                */
  uint64_t scan_alg_ops;     /* their algorithmic int32 ops (1384 * B_tail each)  */
  double scan_kernel_ms;     /* HIP-event kernel time (while profiling is on)     */
  double phase1_ms;          /* host wall ms: plan + launches + stream sync       */
  double gather_ms;          /* host wall ms in the RCCL all-gather phase (0 for  */
                             /*   one device / host combine)                      */
} p1hip_device_stats_t;

int p1hip_get_device_stats(int index, p1hip_device_stats_t *out);

/* Record HIP events (on the library's own stream) around every fast-kernel
 * launch.  Off by default: the events cost a little host time per launch. */
int p1hip_set_profiling(int on);
int p1hip_get_stats(p1hip_stats_t *out);
void p1hip_reset_stats(void);

/* Number of devices currently in use (0 before init). */
int p1hip_device_count(void);

/* Identity of device `index` (as for p1hip_get_device_stats), so a record of
 * an N-GPU run can show that N distinct GPUs took part. */
typedef struct {
  int32_t ordinal;           /* HIP device ordinal                                */
  int32_t cu_count;          /* compute units                                     */
  int32_t clock_khz;         /* peak engine clock                                 */
  int32_t reserved;
  uint64_t hbm_bytes;        /* device memory                                     */
  char pci_bus_id[32];       /* "dddd:bb:dd.f" (hipDeviceGetPCIBusId)             */
  char arch[32];             /* gcnArchName, e.g. "gfx950:sramecc+:xnack-"        */
  unsigned char uuid[16];    /* hipDeviceProp_t.uuid                              */
} p1hip_device_info_t;

int p1hip_device_info(int index, p1hip_device_info_t *out);

/* The RCCL communicator of device `index` (as for p1hip_get_device_stats),
 * as RCCL itself reports it: *nranks = ncclCommCount, *rank =
 * ncclCommUserRank.  A device without a communicator (one device, or the
 * P1HIP_NO_RCCL host combine) gives *nranks = 0, *rank = -1 with rc 0.  With
 * N devices opened by p1hip_init(N) every device reports N ranks and the
 * ranks are 0..N-1 once each: the all-gather inside p1hip_scan spans them
 * all (bench.py refuses to time an N-GPU run for which this does not hold). */
int p1hip_comm_info(int index, int *nranks, int *rank);

/* Layout version of the structs above.  A consumer compiled against this
 * header checks p1hip_abi_version() == P1HIP_ABI_VERSION before reading any
 * p1hip_*_t the library fills in.  History: 4 = p1hip 0.4 (fast_kernel_ms
 * removed from p1hip_stats_t, so the fields after fast_alg_ops moved); 5 =
 * p1hip 0.5 (p1hip_comm_info and this query added; the structs are as in 4);
 * 6 = p1hip 0.6 (p1hip_scan_batch, p1hip_batch_layout, p1hip_get_batch_stats
 * and their structs added; no existing struct changed).  Still 6 with
 * p1hip_scan_batch_wide, p1hip_wide_layout, p1hip_wide_ranges,
 * p1hip_get_wide_stats and p1hip_wide_stats_t, and with the test hook
 * p1hip_scan_tiles and its p1hip_tile_t, and with p1hip_batch_submit,
 * p1hip_batch_wait, p1hip_get_async_stats, p1hip_async_stats_t and
 * P1HIP_ERR_BUSY, and with p1hip_scan_below, p1hip_get_below_stats,
 * p1hip_below_stats_t and the P1HIP_BELOW_* constants, and with
 * p1hip_scan_below_batch, p1hip_below_batch_layout,
 * p1hip_get_below_batch_stats, the test hook p1hip_below_collect and their
 * structs, and with p1hip_scan_below_batch_wide, p1hip_below_wide_layout,
 * p1hip_get_below_wide_stats, p1hip_below_wide_stats_t and the test hook
 * p1hip_below_filter: purely additive, the layout of every existing struct is
 * unchanged. */
#define P1HIP_ABI_VERSION 6
int p1hip_abi_version(void);

const char *p1hip_last_error(void);
const char *p1hip_version(void);

/* Test-only knobs in force for this process.  The library honours its
 * P1HIP_* test knobs (occupancy floor, injected failures, table and launch
 * caps, combine mode ...) only while the master switch P1HIP_TEST_KNOBS=1 is
 * set in the environment; otherwise they are ignored and this returns "".
 * With the switch set it returns "P1HIP_TEST_KNOBS=1" followed by
 * ";NAME=value" for every knob that is set; knobs read at init that the open
 * devices still run with are listed too ("NAME=(init: value)"), even if the
 * environment changed since.  bench.py refuses to time a run for which this
 * is not "".  The string is per thread and valid until the next call from
 * that thread. */
const char *p1hip_test_knobs(void);

/* Release streams, buffers and communicators.  Safe to call twice. */
void p1hip_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif /* P1HIP_H */
