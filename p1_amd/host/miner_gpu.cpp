// miner_gpu.cpp -- the parts of bitcoin.hpp that run on the GPU through
// libp1hip.so's C ABI: bitcoin::Hash (hash.go:13-17) and the miner's scan
// step with miner-side chunking (miner.go:55-66).  Every hash is computed by
// the library; there is no CPU path.  HandleBatch answers many requests
// through one p1hip_scan_batch (or p1hip_scan_batch_wide) call; AnswerPieces
// is the backend of the multi-connection miner's rounds (miner_pool.hpp).
// BelowBatch answers many target searches through one p1hip_scan_below_batch
// (or, `wide`, p1hip_scan_below_batch_wide) call.
#include <string>
#include <vector>

#include "../../include/p1hip.h"
#include "bitcoin.hpp"
#include "miner_pool.hpp"

namespace bitcoin {

static void check(int rc) {
  if (rc != P1HIP_OK) throw HipError(rc, std::string("p1hip: ") + p1hip_last_error());
}

uint64_t Hash(const std::string& msg, uint64_t nonce) {
  uint64_t h = 0;
  check(p1hip_hash(reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), nonce, &h));
  return h;
}

}  // namespace bitcoin

namespace miner {

void ScanChunked(const std::string& msg, uint64_t lower, uint64_t upper, uint64_t chunk, uint64_t* hash,
                 uint64_t* nonce) {
  uint64_t best = UINT64_MAX, bi = 0;
  bool found = false;
  if (chunk == 0) chunk = kDefaultChunk;
  if (lower <= upper) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(msg.data());
    for (uint64_t lo = lower;;) {
      const uint64_t hi = (upper - lo >= chunk) ? lo + (chunk - 1) : upper;
      uint64_t h = 0, n = 0;
      int rc = p1hip_scan(p, msg.size(), lo, hi, &h, &n);
      if (rc != P1HIP_OK) throw bitcoin::HipError(rc, std::string("p1hip_scan: ") + p1hip_last_error());
      // chunks are visited in increasing nonce order: strict '<' keeps the
      // first minimum (miner.go:59); an all-MaxUint64 chunk reads (Max, 0)
      if (h < best) { best = h; bi = n; found = true; }
      if (hi == upper) break;
      lo = hi + 1;
    }
  }
  *hash = best;
  *nonce = found ? bi : 0;
}

bitcoin::Message HandleRequest(const bitcoin::Message& req, uint64_t chunk) {
  uint64_t h = 0, n = 0;
  ScanChunked(req.Data, req.Lower, req.Upper, chunk, &h, &n);
  return bitcoin::NewResult(h, n);
}

std::vector<bitcoin::Message> HandleBatch(const std::vector<bitcoin::Message>& reqs, uint64_t chunk, bool wide) {
  if (chunk == 0) chunk = kDefaultChunk;
  std::vector<bitcoin::Message> res(reqs.size());
  std::vector<p1hip_request_t> q;
  std::vector<size_t> idx;
  for (size_t i = 0; i < reqs.size(); ++i) {
    const bitcoin::Message& m = reqs[i];
    if (m.Lower <= m.Upper && m.Upper - m.Lower >= chunk) {  // more than `chunk` nonces
      res[i] = HandleRequest(m, chunk);
    } else {
      q.push_back({reinterpret_cast<const uint8_t*>(m.Data.data()), m.Data.size(), m.Lower, m.Upper});
      idx.push_back(i);
    }
  }
  std::vector<p1hip_result_t> out(q.size());
  const int rc = wide ? p1hip_scan_batch_wide(q.data(), q.size(), out.data())
                      : p1hip_scan_batch(q.data(), q.size(), out.data());
  if (rc != P1HIP_OK)
    throw bitcoin::HipError(rc, std::string(wide ? "p1hip_scan_batch_wide: " : "p1hip_scan_batch: ") + p1hip_last_error());
  for (size_t j = 0; j < idx.size(); ++j) res[idx[j]] = bitcoin::NewResult(out[j].hash, out[j].nonce);
  return res;
}

std::vector<std::vector<BelowHit>> BelowBatch(const std::vector<BelowJob>& jobs, bool wide) {
  std::vector<p1hip_below_request_t> q;
  q.reserve(jobs.size());
  size_t total = 0;
  for (const BelowJob& j : jobs) {
    uint64_t cap = j.cap;
    if (j.lower > j.upper) cap = 0;
    else if (j.upper - j.lower < cap) cap = j.upper - j.lower + 1;  // at most one hit per nonce
    if (cap > (1ull << 26) || (total += (size_t)cap) > (1ull << 26))
      throw bitcoin::HipError(P1HIP_ERR_ARGS, "below: the caps of one batch add up to more than 2^26 hits");
    q.push_back({reinterpret_cast<const uint8_t*>(j.msg.data()), j.msg.size(), j.lower, j.upper, j.target, (size_t)cap});
  }
  std::vector<p1hip_result_t> hits(total);
  std::vector<size_t> found(q.size(), 0);
  const int rc = wide ? p1hip_scan_below_batch_wide(q.data(), q.size(), hits.data(), hits.size(), found.data())
                      : p1hip_scan_below_batch(q.data(), q.size(), hits.data(), hits.size(), found.data());
  if (rc != P1HIP_OK)
    throw bitcoin::HipError(rc, std::string(wide ? "p1hip_scan_below_batch_wide: " : "p1hip_scan_below_batch: ") +
                                    p1hip_last_error());
  std::vector<std::vector<BelowHit>> out(q.size());
  size_t off = 0;
  for (size_t i = 0; i < q.size(); ++i) {
    for (size_t k = 0; k < found[i]; ++k) out[i].push_back({hits[off + k].hash, hits[off + k].nonce});
    off += q[i].cap;
  }
  return out;
}

void AnswerPieces(const std::vector<Piece>& pieces, bool wide, std::vector<PieceResult>* out) {
  out->assign(pieces.size(), PieceResult());
  if (pieces.empty()) return;
  if (pieces.size() == 1) {  // a light-load round costs what the single-connection miner's scan costs
    const Piece& p = pieces[0];
    const int rc = p1hip_scan(reinterpret_cast<const uint8_t*>(p.msg.data()), p.msg.size(), p.lower, p.upper,
                              &(*out)[0].hash, &(*out)[0].nonce);
    if (rc != P1HIP_OK) throw bitcoin::HipError(rc, std::string("p1hip_scan: ") + p1hip_last_error());
    return;
  }
  std::vector<p1hip_request_t> q;
  q.reserve(pieces.size());
  for (const Piece& p : pieces)
    q.push_back({reinterpret_cast<const uint8_t*>(p.msg.data()), p.msg.size(), p.lower, p.upper});
  std::vector<p1hip_result_t> res(q.size());
  const int rc = wide ? p1hip_scan_batch_wide(q.data(), q.size(), res.data())
                      : p1hip_scan_batch(q.data(), q.size(), res.data());
  if (rc != P1HIP_OK)
    throw bitcoin::HipError(rc, std::string(wide ? "p1hip_scan_batch_wide: " : "p1hip_scan_batch: ") + p1hip_last_error());
  for (size_t i = 0; i < res.size(); ++i) {
    (*out)[i].hash = res[i].hash;
    (*out)[i].nonce = res[i].nonce;
  }
}

uint64_t SubmitPieces(const std::vector<Piece>& pieces, bool wide) {
  std::vector<p1hip_request_t> q;
  q.reserve(pieces.size());
  for (const Piece& p : pieces)
    q.push_back({reinterpret_cast<const uint8_t*>(p.msg.data()), p.msg.size(), p.lower, p.upper});
  p1hip_ticket_t t = 0;
  const int rc = p1hip_batch_submit(q.data(), q.size(), wide ? 1 : 0, &t);  // the messages are borrowed until it returns
  if (rc != P1HIP_OK) throw bitcoin::HipError(rc, std::string("p1hip_batch_submit: ") + p1hip_last_error());
  return t;
}

void CollectPieces(uint64_t handle, std::vector<PieceResult>* out) {
  std::vector<p1hip_result_t> res(out->size());
  const int rc = p1hip_batch_wait(handle, res.data());
  if (rc != P1HIP_OK) throw bitcoin::HipError(rc, std::string("p1hip_batch_wait: ") + p1hip_last_error());
  for (size_t i = 0; i < res.size(); ++i) {
    (*out)[i].hash = res[i].hash;
    (*out)[i].nonce = res[i].nonce;
  }
}

}  // namespace miner
