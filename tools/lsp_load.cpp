// lsp_load -- measurement program: many bitcoin clients in ONE process
// (tools/pool_bench.py).  A p1client process per job would measure fork and
// exec, not the miners behind the server.
//
//   lsp_load <host:port> <clients> <jobs-per-client> <msg-prefix> <maxNonce> [--warm W]
//            [--epoch-limit K] [--epoch-millis M] [--window W] [--copies K] [--connect-copies K]
// Opens <clients> LSP connections; client c sends <jobs-per-client> Requests
// [0, maxNonce] with the message "<msg-prefix><c>-<j>", each after the
// Result of the one before (client.go:35-61).  --warm W: every client first
// sends W untimed Requests ("<msg-prefix>warm<c>-<j>"); the timed ones start
// when all clients have their warm-up answers.  The warm-up runs on the same
// connections on purpose: the server gives a Connect from an address that
// still has a live connection that connection's id again (lsp.cpp, p1.pdf
// 2.1.3), so a second process that happens to get the UDP port of a client
// closed less than EpochLimit epochs ago inherits its sequence numbers, and
// its first Request is taken for a duplicate and never answered.
// Prints one JSON line: wall seconds from the first timed Request to the last
// Result, jobs answered, nonces per job, and a checksum (the xor of every
// timed Result's hash and nonce), so that runs over different miners can be
// compared.  Exit status 1 if a client was disconnected.
#include <errno.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../p1_amd/host/bitcoin.hpp"
#include "../p1_amd/host/lsp.hpp"
#include "../p1_amd/host/lspnet.hpp"

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr,
            "usage: lsp_load <host:port> <clients> <jobs-per-client> <msg-prefix> <maxNonce> [--warm W] [lsp flags]\n");
    return 2;
  }
  lspnet::ConfigureFromEnv();
  lsp::Params prm = lsp::NewParams();
  prm.Copies = lsp::DefaultAppCopies;
  int warm = 0;
  for (int i = 6; i < argc; ++i) {
    if (!strcmp(argv[i], "--epoch-limit") && i + 1 < argc) prm.EpochLimit = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--epoch-millis") && i + 1 < argc) prm.EpochMillis = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--window") && i + 1 < argc) prm.WindowSize = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--copies") && i + 1 < argc) prm.Copies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--connect-copies") && i + 1 < argc) prm.ConnectCopies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--warm") && i + 1 < argc) warm = atoi(argv[++i]);
    else return 2;
  }
  const std::string hostport = argv[1], prefix = argv[4];
  const int clients = atoi(argv[2]), jobs = atoi(argv[3]);
  char* end = nullptr;
  errno = 0;
  const unsigned long long max_nonce = strtoull(argv[5], &end, 10);
  if (clients < 1 || clients > 4096 || jobs < 1 || warm < 0 || errno || *end || !argv[5][0] || argv[5][0] == '-')
    return 2;

  std::vector<std::unique_ptr<lsp::Client>> clis;
  for (int c = 0; c < clients; ++c) {
    std::string err;
    std::unique_ptr<lsp::Client> cli = lsp::NewClient(hostport, prm, &err);
    if (!cli) {
      printf("Failed to connect to server: %s\n", err.c_str());
      return 1;
    }
    clis.push_back(std::move(cli));
  }
  std::vector<uint64_t> sums(clients, 0), answered(clients, 0);
  std::vector<std::thread> threads;
  // the start line of the timed part: the last client to arrive takes the time
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  auto t0 = std::chrono::steady_clock::now();

  auto ask = [&](int c, const std::string& msg, bitcoin::Message* res) {
    std::string buf;
    if (!clis[c]->Write(bitcoin::Marshal(bitcoin::NewRequest(msg, 0, max_nonce))) || !clis[c]->Read(&buf)) return false;
    bitcoin::Unmarshal(buf, res);  // client.go:52-53 ignores the error
    return true;
  };
  for (int c = 0; c < clients; ++c) {
    threads.emplace_back([&, c] {
      bool ok = true;
      bitcoin::Message res;
      for (int j = 0; ok && j < warm; ++j) ok = ask(c, prefix + "warm" + std::to_string(c) + "-" + std::to_string(j), &res);
      {
        std::unique_lock<std::mutex> lk(mu);
        if (++arrived == clients) {
          t0 = std::chrono::steady_clock::now();
          cv.notify_all();
        } else {
          cv.wait(lk, [&] { return arrived == clients; });
        }
      }
      for (int j = 0; ok && j < jobs; ++j) {
        ok = ask(c, prefix + std::to_string(c) + "-" + std::to_string(j), &res);
        if (!ok) break;
        sums[c] ^= res.Hash ^ res.Nonce;
        ++answered[c];
      }
    });
  }
  for (auto& t : threads) t.join();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (auto& cli : clis) cli->Close();
  uint64_t sum = 0, done = 0;
  for (int c = 0; c < clients; ++c) {
    sum ^= sums[c];
    done += answered[c];
  }
  printf("{\"wall_s\": %.6f, \"clients\": %d, \"jobs\": %" PRIu64 ", \"warm_jobs_per_client\": %d, \"nonces_per_job\": %llu, "
         "\"checksum\": \"%016" PRIx64 "\"}\n",
         wall, clients, done, warm, max_nonce + 1, sum);
  return done == (uint64_t)clients * (uint64_t)jobs ? 0 : 1;
}
