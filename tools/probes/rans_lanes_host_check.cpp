// rans_lanes_host_check.cpp — the host coder of the lanes stream (csrc/rans_host.cpp) under the host sanitizers, on the CPU.
//
// A stand-alone program: it links rans_host.cpp and nothing else, needs no GPU and no Python.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/probes/rans_lanes_host_check.cpp \
//       clc_amd/csrc/rans_host.cpp -o /tmp/rans_lanes_host_check && /tmp/rans_lanes_host_check
// It (1) round-trips random inputs — random tables, W, segment lists, symbols inside and far outside their rows — through
// clc_rans_lanes_encode_host and clc_rans_lanes_decoder_*, checking the symbols and the end state (2^31 in every lane, pos == the word
// count), (2) decodes every stream again truncated at a random word and (3) decodes random words of the same lengths: both must return,
// read nothing outside the streams and change nothing they do not own — which is what the sanitizers watch.  Exit status 0: all held.
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/clc_hip.h"

namespace {
struct Tables {
  int rows, stride;
  std::vector<int32_t> cdfs, sizes, offsets;
};

Tables random_tables(std::mt19937_64& g) {
  Tables t;
  t.rows = 1 + (int)(g() % 12);
  t.stride = 4 + (int)(g() % 300);
  t.cdfs.assign((size_t)t.rows * t.stride, 0);
  t.sizes.resize((size_t)t.rows);
  t.offsets.resize((size_t)t.rows);
  for (int r = 0; r < t.rows; ++r) {
    const int size = 3 + (int)(g() % (uint64_t)(t.stride - 2));   // 3 .. stride: at least one symbol and the tail
    t.sizes[(size_t)r] = size;
    t.offsets[(size_t)r] = -(int32_t)(g() % 200);
    // size - 1 strictly increasing steps from 0 to 65536
    std::vector<uint32_t> cut((size_t)size - 2);
    for (auto& c : cut) c = 1 + (uint32_t)(g() % 65535);
    int32_t* row = t.cdfs.data() + (size_t)r * t.stride;
    // distinct sorted cuts: draw, sort, and spread duplicates upward (size - 2 <= 300 cuts in 1 .. 65535 always fit)
    for (size_t i = 0; i < cut.size(); ++i)
      for (size_t j = i + 1; j < cut.size(); ++j)
        if (cut[j] < cut[i]) { const uint32_t s = cut[i]; cut[i] = cut[j]; cut[j] = s; }
    for (size_t i = 1; i < cut.size(); ++i)
      if (cut[i] <= cut[i - 1]) cut[i] = cut[i - 1] + 1;
    for (size_t i = cut.size(); i-- > 0;)
      if (cut[i] > 65535 - (cut.size() - 1 - i)) cut[i] = (uint32_t)(65535 - (cut.size() - 1 - i));
    row[0] = 0;
    for (size_t i = 0; i < cut.size(); ++i) row[i + 1] = (int32_t)cut[i];
    row[size - 1] = 65536;
  }
  return t;
}

int fail(const char* what, int round) {
  fprintf(stderr, "FAILED in round %d: %s (%s)\n", round, what, clc_last_error());
  return 1;
}

long decode_all(clc_rans_lanes_decoder* d, const std::vector<int32_t>& idx, const std::vector<int32_t>& seg, const Tables& t,
                std::vector<int32_t>& out) {
  long at = 0;
  for (int32_t n : seg) {
    if (clc_rans_lanes_decoder_decode(d, idx.data() + at, n, t.cdfs.data(), t.stride, t.rows, t.sizes.data(), t.offsets.data(), out.data() + at) != n)
      return -1;
    at += n;
  }
  return at;
}
}  // namespace

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 300;
  std::mt19937_64 g(20221);
  long symbols = 0, bytes = 0;
  for (int round = 0; round < rounds; ++round) {
    const Tables t = random_tables(g);
    const int W = 1 + (int)(g() % 16), P = (int)(g() % 7);
    std::vector<int32_t> seg((size_t)P);
    long total = 0;
    for (auto& n : seg) { n = (g() % 4 == 0) ? 0 : (int32_t)(g() % 700); total += n; }
    std::vector<int32_t> sym((size_t)total), idx((size_t)total), out((size_t)total);
    for (long i = 0; i < total; ++i) {
      const int r = (int)(g() % (uint64_t)t.rows);
      idx[(size_t)i] = r;
      const int maxv = t.sizes[(size_t)r] - 2;
      int64_t v = (int64_t)(g() % (uint64_t)(maxv + 1));                          // inside, or the tail itself
      const uint64_t kind = g() % 16;
      if (kind == 0) v = -1 - (int64_t)(g() % 40);
      if (kind == 1) v = maxv + (int64_t)(g() % 40);
      if (kind == 2) v = (g() & 1) ? -(int64_t)(g() % 1000000000) : (int64_t)(g() % 1000000000);
      sym[(size_t)i] = (int32_t)(v + t.offsets[(size_t)r]);
    }
    long cap = 0;
    std::vector<long> n_w((size_t)W, 0);
    for (int w = 0; w < W; ++w) {
      for (int32_t n : seg)
        for (long q = w; q * 64 < n; q += W) n_w[(size_t)w] += (q + 1) * 64 <= n ? 64 : n - q * 64;
      cap += clc_rans_lanes_bound(n_w[(size_t)w]);
    }
    std::vector<uint32_t> buf((size_t)cap / 4);   // exactly the documented capacity: one byte more written is a sanitizer report
    std::vector<int32_t> lengths((size_t)W);
    const long nbytes = clc_rans_lanes_encode_host(sym.data(), idx.data(), seg.data(), P, W, t.cdfs.data(), t.stride, t.rows, t.sizes.data(),
                                                   t.offsets.data(), reinterpret_cast<uint8_t*>(buf.data()), cap, lengths.data());
    if (nbytes < 0) return fail("encode", round);
    long sum = 0;
    for (int w = 0; w < W; ++w) {
      if (lengths[(size_t)w] < 512 || lengths[(size_t)w] > clc_rans_lanes_bound(n_w[(size_t)w])) return fail("a wave stream's length", round);
      sum += lengths[(size_t)w];
    }
    if (sum != nbytes) return fail("lengths do not add up", round);
    // the streams in a buffer of exactly their size
    std::vector<uint8_t> streams(reinterpret_cast<uint8_t*>(buf.data()), reinterpret_cast<uint8_t*>(buf.data()) + nbytes);
    clc_rans_lanes_decoder* d = clc_rans_lanes_decoder_create(streams.data(), lengths.data(), W);
    if (!d) return fail("create", round);
    if (decode_all(d, idx, seg, t, out) != total) return fail("decode", round);
    if (out != sym) return fail("the decoded symbols differ", round);
    for (int w = 0; w < W; ++w) {
      uint64_t x[64];
      long pos = 0;
      if (clc_rans_lanes_decoder_state(d, w, x, &pos)) return fail("state", round);
      for (int l = 0; l < 64; ++l)
        if (x[l] != (1ull << 31)) return fail("a lane did not end at 2^31", round);
      if (pos != lengths[(size_t)w] / 4) return fail("pos != the word count", round);
    }
    clc_rans_lanes_decoder_destroy(d);
    // truncated: every wave stream cut at a random word at or after its states
    {
      std::vector<uint8_t> cut;
      std::vector<int32_t> cl((size_t)W);
      long at = 0;
      for (int w = 0; w < W; ++w) {
        const int32_t words = lengths[(size_t)w] / 4;
        cl[(size_t)w] = 4 * (128 + (int32_t)(g() % (uint64_t)(words - 127)));
        cut.insert(cut.end(), streams.begin() + at, streams.begin() + at + cl[(size_t)w]);
        at += lengths[(size_t)w];
      }
      clc_rans_lanes_decoder* dc = clc_rans_lanes_decoder_create(cut.data(), cl.data(), W);
      if (!dc) return fail("create (truncated)", round);
      if (decode_all(dc, idx, seg, t, out) != total) return fail("decode (truncated)", round);
      clc_rans_lanes_decoder_destroy(dc);
    }
    // random words of the same lengths
    {
      std::vector<uint8_t> noise((size_t)nbytes);
      for (auto& b : noise) b = (uint8_t)g();
      clc_rans_lanes_decoder* dn = clc_rans_lanes_decoder_create(noise.data(), lengths.data(), W);
      if (!dn) return fail("create (random words)", round);
      if (decode_all(dn, idx, seg, t, out) != total) return fail("decode (random words)", round);
      clc_rans_lanes_decoder_destroy(dn);
    }
    symbols += total;
    bytes += nbytes;
  }
  printf("rans_lanes_host_check: %d rounds, %ld symbols, %ld stream bytes: round trips exact, end states hold, truncated and random words decode in bounds\n",
         rounds, symbols, bytes);
  return 0;
}
