// p1miner -- the miner's Request -> Result loop (miner.go:49-67), GPU-backed
// through libp1hip.so, over LSP (the reference's transport) or stdio.
// Requests/results are encoding/json bitcoin.Message bytes (miner.go:55,66).
//
//   p1miner lsp <host:port> [--device N] [--chunk C] [--epoch-limit K]
//           [--epoch-millis M] [--window W] [--copies K] [--connect-copies K]
//                                        miner.go:13-73: connect, send Join,
//                                        then Read -> scan -> Write until the
//                                        connection is lost.  The scan runs on
//                                        this thread while the LSP event loop
//                                        keeps heartbeating, so a long GPU job
//                                        never trips the epoch limit.
//   p1miner lsp <host:port> --conns C [--wide] [--linger-us U] [--round-log FILE] [--inflight N]
//           [--stats] [the flags above]  one process, C connections (1..256),
//                                        each a miner to the server; their jobs
//                                        are answered in rounds, one piece of at
//                                        most --chunk nonces of every connection's
//                                        job per GPU call (miner_pool.hpp): one
//                                        piece through p1hip_scan, more through
//                                        p1hip_scan_batch, or, with --wide,
//                                        p1hip_scan_batch_wide.  --linger-us U:
//                                        wait up to U us for more jobs before a
//                                        round (default 0).  --round-log FILE:
//                                        one line per round, its index and then
//                                        conn:lower:upper per piece.  --stats:
//                                        one JSON line on stdout at exit.
//                                        --inflight N (1..4, default 1): up to
//                                        N rounds outstanding, each through
//                                        p1hip_batch_submit / p1hip_batch_wait,
//                                        so the next round is cut and submitted
//                                        and Results are written while the GPU
//                                        runs the last one.  Ends
//                                        when every connection is lost, or on
//                                        SIGTERM / SIGINT.
//
//   p1miner scan <msg> <lower> <upper>   prints "Result <hash> <nonce>"
//                                        (the client's output, client.go:59-61)
//   p1miner scan <msg> <lower> <upper> --below <target> [--count N]
//                                        every nonce of [lower, upper] whose hash
//                                        is at or below <target>, the first N of
//                                        them (default 1), through
//                                        p1hip_scan_below: one "Result <hash>
//                                        <nonce>" line per hit in nonce order;
//                                        exits 0 with no line when there is none
//   p1miner below [--device N] [--batch B] [--hard]
//                                        one target search per stdin line,
//                                        "<msg-hex|-> <lower> <upper> <target>
//                                        <cap>" ("-": the empty message); the
//                                        lines are collected and answered
//                                        together, in order, through one
//                                        p1hip_scan_below_batch call, on the B-th
//                                        line (default 256), on an empty line
//                                        (itself not answered) or at EOF.  Every
//                                        line is answered with "Hits <found>" and
//                                        then <found> lines "Result <hash>
//                                        <nonce>" in nonce order.  A line that
//                                        does not parse ends the program with
//                                        status 1 after the lines before it are
//                                        answered.  --hard: through
//                                        p1hip_scan_below_batch_wide, which also
//                                        coalesces the hard-target searches; the
//                                        lines read and written are the same.
//   p1miner hash <msg> <nonce>           prints bitcoin.Hash(msg, nonce)
//   p1miner serve [--device N] [--chunk C] [--batch B [--wide]]
//                                        one JSON Message per stdin line; every
//                                        line is answered with one JSON Result
//                                        line (miner.go:49-67 scans whatever it
//                                        decoded, as Go's Unmarshal leaves it).
//                                        --batch B (B > 1): request lines are
//                                        collected and answered together, in
//                                        order, through one p1hip_scan_batch
//                                        call, on the B-th line, on an empty
//                                        line (itself not answered) or at EOF;
//                                        --wide: through p1hip_scan_batch_wide,
//                                        so requests of up to 2^24 nonces share
//                                        launches too (no effect without --batch)
//   p1miner json                         re-marshals stdin JSON lines (no GPU;
//                                        wire-format tests): "ERROR" for a
//                                        syntax error, "TYPEERROR\t" before
//                                        Go's partial decode on a type error
//   p1miner lsp-json                     re-marshals stdin lsp.Message JSON lines
//                                        (lsp/message.go; no GPU)
//   p1miner lsp-wrap <connID> <seq>      each stdin bitcoin.Message JSON line ->
//                                        the LSP Data datagram that carries it
//                                        (miner.go:66 client.Write), seq counting up
//   p1miner lsp-unwrap                   LSP Data datagram lines -> the bitcoin
//                                        message in their payload (miner.go:50-55)
#include <errno.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/p1hip.h"
#include "bitcoin.hpp"
#include "gojson.hpp"
#include "lsp.hpp"
#include "lsp_message.hpp"
#include "lspnet.hpp"
#include "miner_pool.hpp"

static int usage() {
  fprintf(stderr,
          "usage: p1miner scan <msg> <lower> <upper> [--below <target> [--count N]] | below [--device N] [--batch B] [--hard] | "
          "hash <msg> <nonce> | "
          "serve [--device N] [--chunk C] [--batch B [--wide]] | lsp <host:port> [--device N] [--chunk C] [--epoch-limit K] "
          "[--epoch-millis M] [--window W] [--copies K] [--connect-copies K] "
          "[--conns C [--wide] [--linger-us U] [--round-log FILE] [--stats] [--inflight N]] | json | lsp-json | lsp-wrap <connID> <seq> | lsp-unwrap\n");
  return 2;
}

static bool parse_u64(const char* s, uint64_t* v) {
  char* end = nullptr;
  if (!s || !*s || *s == '-') return false;
  errno = 0;
  unsigned long long r = strtoull(s, &end, 10);
  if (errno || *end) return false;
  *v = r;
  return true;
}

// p1miner scan ... --below <target> [--count N]: the first `count` hits, asked
// for in calls of at most 2^16 hits, each resuming after the last one's last hit.
static int run_below(const char* msg, uint64_t lo, uint64_t hi, uint64_t target, uint64_t count) {
  std::vector<p1hip_result_t> hits((size_t)(count < 65536 ? count : 65536));
  while (count > 0 && lo <= hi) {
    const size_t cap = (size_t)(count < hits.size() ? count : hits.size());
    size_t found = 0;
    if (p1hip_scan_below((const uint8_t*)msg, strlen(msg), lo, hi, target, cap, hits.data(), &found) != P1HIP_OK) {
      fprintf(stderr, "p1hip_scan_below: %s\n", p1hip_last_error());
      return 1;
    }
    for (size_t i = 0; i < found; ++i) printf("Result %" PRIu64 " %" PRIu64 "\n", hits[i].hash, hits[i].nonce);
    if (found < cap || hits[found - 1].nonce == UINT64_MAX) break;
    count -= found;
    lo = hits[found - 1].nonce + 1;
  }
  p1hip_shutdown();
  return 0;
}

// One line of `p1miner below`: "<msg-hex|-> <lower> <upper> <target> <cap>".
static bool parse_below_line(const std::string& line, miner::BelowJob* job) {
  std::vector<std::string> f;
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
    size_t j = i;
    while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
    if (j > i) f.push_back(line.substr(i, j - i));
    i = j;
  }
  if (f.size() != 5) return false;
  job->msg.clear();
  if (f[0] != "-") {
    if (f[0].size() % 2) return false;
    for (size_t k = 0; k < f[0].size(); k += 2) {
      int v = 0;
      for (int d = 0; d < 2; ++d) {
        const char c = f[0][k + d];
        const int x = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (x < 0) return false;
        v = v * 16 + x;
      }
      job->msg.push_back((char)v);
    }
  }
  return parse_u64(f[1].c_str(), &job->lower) && parse_u64(f[2].c_str(), &job->upper) &&
         parse_u64(f[3].c_str(), &job->target) && parse_u64(f[4].c_str(), &job->cap);
}

// p1miner below: batches of target searches through miner::BelowBatch.  The
// device is opened by the first batch that needs one (or, with --device, by
// the first batch).
static int run_below_batches(int dev, uint64_t batch, bool wide) {
  std::vector<miner::BelowJob> jobs;
  bool opened = false;
  auto flush = [&]() -> bool {
    if (dev >= 0 && !opened) {
      if (p1hip_init_devices(&dev, 1) != P1HIP_OK) {
        fprintf(stderr, "p1hip init: %s\n", p1hip_last_error());
        return false;
      }
      opened = true;
    }
    for (const std::vector<miner::BelowHit>& hits : miner::BelowBatch(jobs, wide)) {
      printf("Hits %zu\n", hits.size());
      for (const miner::BelowHit& h : hits) printf("Result %" PRIu64 " %" PRIu64 "\n", h.hash, h.nonce);
    }
    fflush(stdout);
    jobs.clear();
    return true;
  };
  std::string line;
  uint64_t lineno = 0;
  int rc = 0;
  while (std::getline(std::cin, line)) {
    ++lineno;
    if (line.empty()) {  // flush now; the empty line itself is not answered
      if (!jobs.empty() && !flush()) return 1;
      continue;
    }
    miner::BelowJob job;
    if (!parse_below_line(line, &job)) {
      fprintf(stderr, "below: line %" PRIu64 " is not \"<msg-hex|-> <lower> <upper> <target> <cap>\"\n", lineno);
      rc = 1;
      break;
    }
    jobs.push_back(job);
    if (jobs.size() >= batch && !flush()) return 1;
  }
  if (!jobs.empty() && !flush()) return 1;
  p1hip_shutdown();
  return rc;
}

// p1miner lsp --conns C: the GPU is open; run the pool (miner_pool.hpp) over
// miner::AnswerPieces, print the statistics, release the GPU.
static int run_pool(const std::string& hostport, const lsp::Params& prm, int conns, uint64_t chunk, long linger_us,
                    bool wide, int inflight, const std::string& round_log, bool want_stats) {
  miner::PoolStats st;
  std::string err;
  miner::AsyncBackend async;
  async.Submit = [wide](const std::vector<miner::Piece>& pieces) { return miner::SubmitPieces(pieces, wide); };
  async.Collect = [](uint64_t h, std::vector<miner::PieceResult>* out) { miner::CollectPieces(h, out); };
  const int rc = miner::RunPool(
      hostport, prm, conns, chunk, linger_us,
      [wide](const std::vector<miner::Piece>& pieces, std::vector<miner::PieceResult>* out) {
        miner::AnswerPieces(pieces, wide, out);
      },
      async, inflight, round_log, &st, &err);
  if (rc != 0) {
    printf("Failed to join with server: %s\n", err.c_str());
    return 1;
  }
  if (want_stats) {
    p1hip_batch_stats_t b = {};
    p1hip_wide_stats_t w = {};
    p1hip_get_batch_stats(&b);
    p1hip_get_wide_stats(&w);
    printf("{%s, \"batch\": {\"calls\": %" PRIu64 ", \"requests\": %" PRIu64 ", \"coalesced\": %" PRIu64
           ", \"individual\": %" PRIu64 ", \"empty\": %" PRIu64 ", \"launches\": %" PRIu64 ", \"tiles\": %" PRIu64
           ", \"nonces\": %" PRIu64 ", \"wall_ms\": %.3f}, \"wide\": {\"calls\": %" PRIu64 ", \"requests\": %" PRIu64
           ", \"empty\": %" PRIu64 ", \"small\": %" PRIu64 ", \"wide\": %" PRIu64 ", \"individual\": %" PRIu64
           ", \"scan_launches\": %" PRIu64 ", \"scan_segments\": %" PRIu64 ", \"generic_launches\": %" PRIu64
           ", \"generic_segments\": %" PRIu64 ", \"tiles\": %" PRIu64 ", \"nonces\": %" PRIu64 ", \"wall_ms\": %.3f}}\n",
           miner::StatsJsonFields(st).c_str(), b.calls, b.requests, b.coalesced, b.individual, b.empty, b.launches, b.tiles,
           b.nonces, b.wall_ms, w.calls, w.requests, w.empty, w.small, w.wide, w.individual, w.scan_launches,
           w.scan_segments, w.generic_launches, w.generic_segments, w.tiles, w.nonces, w.wall_ms);
    fflush(stdout);
  }
  p1hip_shutdown();
  return 0;
}

// miner.go:13-31 (joinWithServer) + miner.go:33-73 (main loop)
static int run_lsp(int argc, char** argv) {
  const std::string hostport = argv[2];
  int dev = -1;
  uint64_t chunk = miner::kDefaultChunk;
  uint64_t conns = 0, linger_us = 0, inflight = 1;
  bool wide = false, want_stats = false;
  std::string round_log;
  lsp::Params prm = lsp::NewParams();
  prm.Copies = lsp::DefaultAppCopies;
  for (int i = 3; i < argc; ++i) {
    if (!strcmp(argv[i], "--device") && i + 1 < argc) dev = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--inflight") && i + 1 < argc) { if (!parse_u64(argv[++i], &inflight) || inflight < 1 || inflight > P1HIP_MAX_INFLIGHT) return usage(); }
    else if (!strcmp(argv[i], "--conns") && i + 1 < argc) { if (!parse_u64(argv[++i], &conns) || conns < 1 || conns > 256) return usage(); }
    else if (!strcmp(argv[i], "--linger-us") && i + 1 < argc) { if (!parse_u64(argv[++i], &linger_us) || linger_us > 60000000) return usage(); }
    else if (!strcmp(argv[i], "--round-log") && i + 1 < argc) round_log = argv[++i];
    else if (!strcmp(argv[i], "--wide")) wide = true;
    else if (!strcmp(argv[i], "--stats")) want_stats = true;
    else if (!strcmp(argv[i], "--chunk") && i + 1 < argc) { if (!parse_u64(argv[++i], &chunk)) return usage(); }
    else if (!strcmp(argv[i], "--epoch-limit") && i + 1 < argc) prm.EpochLimit = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--epoch-millis") && i + 1 < argc) prm.EpochMillis = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--window") && i + 1 < argc) prm.WindowSize = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--copies") && i + 1 < argc) prm.Copies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--connect-copies") && i + 1 < argc) prm.ConnectCopies = atoi(argv[++i]);
    else return usage();
  }
  // the pool's flags mean nothing to the single-connection loop
  if (conns == 0 && (wide || want_stats || linger_us || inflight != 1 || !round_log.empty())) return usage();
  // open the GPU before joining, so the first request does not pay for it
  int rc = dev >= 0 ? p1hip_init_devices(&dev, 1) : p1hip_init(0, nullptr);
  if (rc != P1HIP_OK) { fprintf(stderr, "p1hip init: %s\n", p1hip_last_error()); return 1; }
  std::string err;
  if (conns) return run_pool(hostport, prm, (int)conns, chunk, (long)linger_us, wide, (int)inflight, round_log, want_stats);
  std::unique_ptr<lsp::Client> cli = lsp::NewClient(hostport, prm, &err);
  if (!cli) {
    printf("Failed to join with server: %s\n", err.c_str());
    return 1;
  }
  if (!cli->Write(bitcoin::Marshal(bitcoin::NewJoin()), &err)) {
    cli->Close();
    printf("Failed to join with server: %s\n", err.c_str());
    return 1;
  }
  for (;;) {
    std::string buf;
    if (!cli->Read(&buf)) break;
    bitcoin::Message req;
    bitcoin::Unmarshal(buf, &req);  // miner.go:54-55: a fresh Message, the error ignored (partial decode kept)
    const bitcoin::Message res = miner::HandleRequest(req, chunk);
    if (!cli->Write(bitcoin::Marshal(res))) break;
  }
  cli->Close();  // miner.go:47 (defer miner.Close())
  p1hip_shutdown();
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  const std::string cmd = argv[1];
  lspnet::ConfigureFromEnv();
  try {
    if (cmd == "lsp" && argc >= 3) return run_lsp(argc, argv);
    if (cmd == "scan" && argc == 5) {
      uint64_t lo, hi, h, n;
      if (!parse_u64(argv[3], &lo) || !parse_u64(argv[4], &hi)) return usage();
      miner::ScanChunked(argv[2], lo, hi, miner::kDefaultChunk, &h, &n);
      printf("Result %" PRIu64 " %" PRIu64 "\n", h, n);
      return 0;
    }
    if (cmd == "scan" && argc > 5) {
      uint64_t lo, hi, target = 0, count = 1;
      bool below = false;
      if (!parse_u64(argv[3], &lo) || !parse_u64(argv[4], &hi)) return usage();
      for (int i = 5; i < argc; ++i) {
        if (!strcmp(argv[i], "--below") && i + 1 < argc) { if (!parse_u64(argv[++i], &target)) return usage(); below = true; }
        else if (!strcmp(argv[i], "--count") && i + 1 < argc) { if (!parse_u64(argv[++i], &count) || count == 0) return usage(); }
        else return usage();
      }
      if (!below) return usage();  // --count means nothing to the minimum scan
      return run_below(argv[2], lo, hi, target, count);
    }
    if (cmd == "below") {
      int dev = -1;
      uint64_t batch = 256, d = 0;
      bool wide = false;
      for (int i = 2; i < argc; ++i) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) { if (!parse_u64(argv[++i], &d) || d > 1023) return usage(); dev = (int)d; }
        else if (!strcmp(argv[i], "--batch") && i + 1 < argc) { if (!parse_u64(argv[++i], &batch) || batch == 0) return usage(); }
        else if (!strcmp(argv[i], "--hard")) wide = true;  // `below --wide` stays a usage error
        else return usage();
      }
      return run_below_batches(dev, batch, wide);
    }
    if (cmd == "hash" && argc == 4) {
      uint64_t n;
      if (!parse_u64(argv[3], &n)) return usage();
      printf("%" PRIu64 "\n", bitcoin::Hash(argv[2], n));
      return 0;
    }
    if (cmd == "json") {
      std::string line;
      while (std::getline(std::cin, line)) {
        bitcoin::Message m;
        const int st = bitcoin::UnmarshalStatus(line, &m);
        if (st == gojson::kSyntaxError) { printf("ERROR\n"); continue; }
        // fwrite, not %s: a decoded string may hold NUL bytes
        const std::string o = (st == gojson::kTypeError ? "TYPEERROR\t" : "") + bitcoin::Marshal(m) + "\t" + m.String() + "\n";
        fwrite(o.data(), 1, o.size(), stdout);
      }
      return 0;
    }
    if (cmd == "lsp-json") {
      std::string line;
      while (std::getline(std::cin, line)) {
        lsp::Message m;
        const int st = lsp::UnmarshalStatus(line, &m);
        if (st == gojson::kSyntaxError) { printf("ERROR\n"); continue; }
        // fwrite, not %s: a decoded string may hold NUL bytes
        const std::string o = (st == gojson::kTypeError ? "TYPEERROR\t" : "") + lsp::Marshal(m) + "\t" + m.String() + "\n";
        fwrite(o.data(), 1, o.size(), stdout);
      }
      return 0;
    }
    if (cmd == "lsp-wrap" && argc == 4) {
      char* end = nullptr;
      const long long conn = strtoll(argv[2], &end, 10);
      if (*end) return usage();
      long long seq = strtoll(argv[3], &end, 10);
      if (*end) return usage();
      std::string line;
      while (std::getline(std::cin, line)) {
        bitcoin::Message m;
        if (!bitcoin::Unmarshal(line, &m)) { printf("ERROR\n"); continue; }
        const std::string payload = bitcoin::Marshal(m);
        printf("%s\n", lsp::Marshal(lsp::NewData(conn, seq++, (int64_t)payload.size(), payload)).c_str());
      }
      return 0;
    }
    if (cmd == "lsp-unwrap") {
      std::string line;
      while (std::getline(std::cin, line)) {
        lsp::Message d;
        bitcoin::Message m;
        if (!lsp::Unmarshal(line, &d) || d.Type != lsp::MsgData ||
            !bitcoin::Unmarshal(std::string(d.Payload.begin(), d.Payload.end()), &m)) {
          printf("ERROR\n");
          continue;
        }
        printf("%s\n", bitcoin::Marshal(m).c_str());
      }
      return 0;
    }
    if (cmd == "serve") {
      int dev = -1;
      uint64_t chunk = miner::kDefaultChunk, batch = 1;
      bool wide = false;
      for (int i = 2; i < argc; ++i) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) dev = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--chunk") && i + 1 < argc) { if (!parse_u64(argv[++i], &chunk)) return usage(); }
        else if (!strcmp(argv[i], "--batch") && i + 1 < argc) { if (!parse_u64(argv[++i], &batch) || batch == 0) return usage(); }
        else if (!strcmp(argv[i], "--wide")) wide = true;
        else return usage();
      }
      int rc = dev >= 0 ? p1hip_init_devices(&dev, 1) : p1hip_init(0, nullptr);
      if (rc != P1HIP_OK) { fprintf(stderr, "p1hip init: %s\n", p1hip_last_error()); return 1; }
      std::string line;
      if (batch > 1) {
        // the same decode per line as below; the answers of a batch are
        // written together, one Result line per request line, in order
        std::vector<bitcoin::Message> reqs;
        auto flush = [&]() {
          for (const bitcoin::Message& res : miner::HandleBatch(reqs, chunk, wide)) printf("%s\n", bitcoin::Marshal(res).c_str());
          fflush(stdout);
          reqs.clear();
        };
        while (std::getline(std::cin, line)) {
          if (line.empty()) {  // flush now; the empty line itself is not answered
            if (!reqs.empty()) flush();
            continue;
          }
          bitcoin::Message req;
          bitcoin::Unmarshal(line, &req);
          reqs.push_back(req);
          if (reqs.size() >= batch) flush();
        }
        if (!reqs.empty()) flush();
        p1hip_shutdown();
        return 0;
      }
      while (std::getline(std::cin, line)) {
        // miner.go:54-55 decodes into a fresh Message and ignores the error,
        // then scans [Lower, Upper] whatever the Type: a line with a type
        // error scans what Go's partial decode holds, a line that is not JSON
        // the one-nonce request ("", [0, 0]); every line is answered, so a
        // server never waits on a miner that stays silent.
        bitcoin::Message req;
        bitcoin::Unmarshal(line, &req);
        bitcoin::Message res = miner::HandleRequest(req, chunk);
        printf("%s\n", bitcoin::Marshal(res).c_str());
        fflush(stdout);
      }
      p1hip_shutdown();
      return 0;
    }
  } catch (const bitcoin::HipError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return usage();
}
