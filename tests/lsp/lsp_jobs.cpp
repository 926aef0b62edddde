// lsp_jobs -- test client: ONE LSP connection that sends several Requests,
// each after the Result of the one before (client.go:35-61 in a loop), with
// any Lower and Upper -- p1client always sends Lower = 0, so it cannot ask for
// an empty range (Lower > Upper).
//
//   lsp_jobs <host:port> [--epoch-limit K] [--epoch-millis M] [--window W] [--copies K] [--connect-copies K]
//            -- <msg> <lower> <upper> [<msg> <lower> <upper> ...]
// Prints "Result <hash> <nonce>" per job, in order, or "Disconnected" and
// exit status 1 (client.go:64-66).  P1LSP_* env vars inject loss (lspnet.hpp).
#include <errno.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>

#include "../../p1_amd/host/bitcoin.hpp"
#include "../../p1_amd/host/lsp.hpp"
#include "../../p1_amd/host/lspnet.hpp"

static bool parse_u64(const char* s, uint64_t* v) {
  char* end = nullptr;
  if (!s || !*s || *s == '-') return false;
  errno = 0;
  unsigned long long r = strtoull(s, &end, 10);
  if (errno || *end) return false;
  *v = r;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  lspnet::ConfigureFromEnv();
  lsp::Params prm = lsp::NewParams();
  prm.Copies = lsp::DefaultAppCopies;  // like p1client
  int i = 2;
  for (; i < argc && strcmp(argv[i], "--"); ++i) {
    if (!strcmp(argv[i], "--epoch-limit") && i + 1 < argc) prm.EpochLimit = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--epoch-millis") && i + 1 < argc) prm.EpochMillis = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--window") && i + 1 < argc) prm.WindowSize = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--copies") && i + 1 < argc) prm.Copies = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--connect-copies") && i + 1 < argc) prm.ConnectCopies = atoi(argv[++i]);
    else return 2;
  }
  if (i >= argc || (argc - i - 1) % 3 != 0 || argc - i - 1 == 0) return 2;
  std::string err;
  std::unique_ptr<lsp::Client> cli = lsp::NewClient(argv[1], prm, &err);
  if (!cli) {
    printf("Failed to connect to server: %s\n", err.c_str());
    return 1;
  }
  for (int k = i + 1; k + 2 < argc; k += 3) {
    uint64_t lo = 0, hi = 0;
    if (!parse_u64(argv[k + 1], &lo) || !parse_u64(argv[k + 2], &hi)) return 2;
    std::string buf;
    if (!cli->Write(bitcoin::Marshal(bitcoin::NewRequest(argv[k], lo, hi))) || !cli->Read(&buf)) {
      printf("Disconnected\n");
      fflush(stdout);
      return 1;
    }
    bitcoin::Message res;
    bitcoin::Unmarshal(buf, &res);  // client.go:52-53 ignores the error
    printf("Result %" PRIu64 " %" PRIu64 "\n", res.Hash, res.Nonce);
    fflush(stdout);
  }
  cli->Close();
  return 0;
}
