// Test driver for demuxlet_amd/csrc/dmx_inflate_core.hpp, the decoder core that the device kernel k_bgzf_inflate instantiates
// (built by tests/test_gpu_inflate_cpu.py, once with -fsanitize=address,undefined and once with -O2, and run as a program).
// The host instantiation keeps every array the core touches in a heap buffer of exactly the size the contract allows — the tables,
// the code-length arrays, the padded input slot ((in_len + 11) / 4 words) and the output (out_len bytes) — so that the sanitizer
// sees any access outside them.  Three parts:
//   valid    streams zlib's deflate made, and hand-made ones (one-code distance sets; distance 32 768): accepted as zlib accepts, with its bytes
//   damaged  seeded bit flips, truncations and wrong sizes: status 0 => zlib accepts the stream at exactly out_len with the same bytes
//   file     (argv[1], optional) a corpus written by tests/inflate_corpus.py, same rule; argv[2]: one status byte per stream goes there
// Prints one line of counts per part; exit code 0 = all good.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dmx_inflate_core.hpp"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

// ---- the host policy: exact-size heap arrays, plain loops
struct HostPolicy {
  std::unique_ptr<uint32_t[]> lit_{new uint32_t[dmxzc::kLitCap]}, dist_{new uint32_t[dmxzc::kDistCap]}, ct_{new uint32_t[dmxzc::kClCap]};
  std::unique_ptr<uint8_t[]> lens_{new uint8_t[dmxzc::kLensCap]}, submax_{new uint8_t[dmxzc::kSubmaxCap]}, cl_{new uint8_t[19]};
  std::unique_ptr<uint16_t[]> count_{new uint16_t[dmxzc::kCountCap]};
  uint32_t *lit = lit_.get(), *dist = dist_.get(), *ct = ct_.get();
  uint8_t *lens = lens_.get(), *submax = submax_.get(), *cl = cl_.get();
  uint16_t* count = count_.get();
  uint8_t* out = nullptr;
  void sync() {}
  void fill32(uint32_t* t, uint32_t first, uint32_t step, uint32_t limit, uint32_t v) { for (uint32_t i = first; i < limit; i += step) t[i] = v; }
  void fill16(uint16_t* t, uint32_t n, uint16_t v) { for (uint32_t i = 0; i < n; ++i) t[i] = v; }
  void fill8(uint8_t* t, uint32_t n, uint8_t v) { for (uint32_t i = 0; i < n; ++i) t[i] = v; }
  void put(uint32_t pos, uint8_t v) { out[pos] = v; }
  void copy_in(uint32_t pos, const uint8_t* src, uint32_t n) { for (uint32_t i = 0; i < n; ++i) out[pos + i] = src[i]; }
  void copy_match(uint32_t pos, uint32_t d, uint32_t len) { for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos - d + (d < len ? i % d : i)]; }
};

// one member through the core: fresh exact-size buffers for the slot and the output
static int32_t core_inflate(const uint8_t* z, size_t in_len, std::vector<uint8_t>& out, size_t out_len) {
  static HostPolicy P;
  if (in_len > dmxzc::kMaxIn || out_len > dmxzc::kMaxOut) return dmxzc::ST_LIMIT;
  const size_t n_words = (in_len + 8 + 3) / 4;
  std::unique_ptr<uint32_t[]> slot(new uint32_t[n_words]);
  memset(slot.get(), 0xA5, n_words * 4);             // not zero: bytes past in_len must not matter
  memcpy(slot.get(), z, in_len);
  std::unique_ptr<uint8_t[]> o(new uint8_t[out_len]);
  memset(o.get(), 0xEE, out_len);
  P.out = o.get();
  const int32_t st = dmxzc::inflate_member(P, slot.get(), (uint32_t)in_len, (uint32_t)out_len);
  out.assign(o.get(), o.get() + out_len);
  return st;
}

static std::vector<uint8_t> make_data(int kind, size_t n) {
  std::vector<uint8_t> d(n);
  switch (kind) {
    case 0: for (auto& b : d) b = (uint8_t)rnd(); break;                                   // incompressible
    case 1: for (auto& b : d) b = "ACGT"[rnd() & 3]; break;                                // four symbols
    case 2: for (size_t i = 0; i < n; ++i) d[i] = (uint8_t)(i < 7 ? rnd() : d[i - 1 - rnd() % 7]); break;   // distances 1..7
    case 3: for (auto& b : d) b = 0; break;                                                // one long run (distance 1, length 258)
    case 4: {                                                                              // BAM-like: short repeats + noisy bytes
      size_t i = 0;
      while (i < n) {
        if (i > 300 && (rnd() & 3)) { const size_t len = 3 + rnd() % 12, dist = 1 + rnd() % 300; for (size_t k = 0; k < len && i < n; ++k, ++i) d[i] = d[i - dist]; }
        else d[i++] = (uint8_t)(33 + rnd() % 42);
      }
      break;
    }
    case 5: for (size_t i = 0; i < n; ++i) d[i] = (uint8_t)((i * 2654435761u) >> 13); break;   // structured, long matches far back
    case 6: for (auto& b : d) { uint32_t r = rnd(), s = 0; while ((r & 1u) && s < 40) { r >>= 1; ++s; } b = (uint8_t)s; } break;   // geometric symbol frequencies: 15-bit codes
    default: {                                                                             // a 32 000-byte period: zlib finds length-258 matches at distance 32 000
      for (size_t i = 0; i < n; ++i) d[i] = i < 32000 ? (uint8_t)rnd() : d[i - 32000];       // (its limit is 32 768 - 262; 32 768 itself is hand-made in main)
    }
  }
  return d;
}

// raw deflate of d; `pieces` > 1 writes it in that many parts with Z_FULL_FLUSH between them (several blocks, empty stored blocks)
static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t>& d, int level, int strategy, int pieces = 1) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy);
  std::vector<uint8_t> out(deflateBound(&zs, (uLong)d.size()) + 64 + 16 * (size_t)pieces);
  zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
  size_t at = 0;
  for (int q = 0; q < pieces; ++q) {
    const size_t end = q + 1 == pieces ? d.size() : d.size() * (size_t)(q + 1) / (size_t)pieces;
    zs.next_in = (Bytef*)d.data() + at; zs.avail_in = (uInt)(end - at);
    deflate(&zs, q + 1 == pieces ? Z_FINISH : Z_FULL_FLUSH);
    at = end;
  }
  out.resize(zs.total_out);
  deflateEnd(&zs);
  return out;
}

static bool zlib_inflate(const uint8_t* in, size_t n, std::vector<uint8_t>& out, size_t want) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  inflateInit2(&zs, -15);
  out.assign(want + 1, 0);
  zs.next_in = (Bytef*)in; zs.avail_in = (uInt)n;
  zs.next_out = out.data(); zs.avail_out = (uInt)want;
  const int rc = inflate(&zs, Z_FINISH);
  inflateEnd(&zs);
  out.resize(want);
  return rc == Z_STREAM_END && zs.avail_out == 0;
}

struct Stream { std::vector<uint8_t> z, d; };
static size_t n_ok = 0, n_bad = 0;

static void check_valid(const Stream& s, const char* what) {
  std::vector<uint8_t> out;
  const int32_t st = core_inflate(s.z.data(), s.z.size(), out, s.d.size());
  if (st == 0 && out == s.d) ++n_ok;
  else { ++n_bad; fprintf(stderr, "MISMATCH %s: n %zu, status %d\n", what, s.d.size(), (int)st); }
}

// damaged: returns 0 = zlib rejects, 1 = zlib accepts with the original's bytes, 2 = zlib accepts with other bytes
static size_t n_dam = 0, n_dam_acc = 0, n_cls[3] = {0, 0, 0};
static void check_damaged(const uint8_t* z, size_t zl, size_t out_len, const std::vector<uint8_t>& orig, const char* what) {
  std::vector<uint8_t> mine, zo;
  const int32_t st = core_inflate(z, zl, mine, out_len);
  const bool theirs = zlib_inflate(z, zl, zo, out_len);
  ++n_dam;
  ++n_cls[!theirs ? 0 : (out_len == orig.size() && zo == orig ? 1 : 2)];
  if (st == 0) {
    ++n_dam_acc;
    if (!theirs || mine != zo) { ++n_bad; fprintf(stderr, "damaged stream (%s) accepted with other bytes than zlib: in %zu out %zu\n", what, zl, out_len); }
  }
}

static int run_file(const char* path, const char* status_path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 1; }
  size_t n = 0, acc = 0, bad = 0;
  std::vector<uint8_t> statuses;
  for (;;) {
    uint32_t h[2];
    if (fread(h, 4, 2, f) != 2) break;
    std::vector<uint8_t> z(h[0]), mine, zo;
    if (h[0] && fread(z.data(), 1, h[0], f) != h[0]) { fprintf(stderr, "short corpus file\n"); fclose(f); return 1; }
    const int32_t st = core_inflate(z.data(), z.size(), mine, h[1]);
    statuses.push_back((uint8_t)st);
    ++n;
    if (st == 0) {
      ++acc;
      if (!(h[1] <= 65536 && zlib_inflate(z.data(), z.size(), zo, h[1])) || mine != zo) { ++bad; fprintf(stderr, "file stream %zu accepted with other bytes than zlib\n", n - 1); }
    }
  }
  fclose(f);
  if (status_path) { FILE* g = fopen(status_path, "wb"); if (!g) return 1; fwrite(statuses.data(), 1, statuses.size(), g); fclose(g); }
  printf("file streams %zu, accepted %zu, failures %zu\n", n, acc, bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  std::vector<Stream> valid;
  // ---- valid: inflate_check.cpp's shape (six kinds x 13 sizes x five levels x four strategies) ...
  static const size_t sizes[] = {0, 1, 2, 7, 64, 287, 288, 289, 300, 1000, 4096, 65280, 65536};
  for (int kind = 0; kind < 6; ++kind)
    for (size_t n : sizes)
      for (int level : {0, 1, 4, 6, 9})
        for (int strategy : {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE}) {
          Stream s; s.d = make_data(kind, n); s.z = deflate_raw(s.d, level, strategy);
          valid.push_back(std::move(s));
        }
  const size_t n_shape = valid.size();
  // ... and: more sizes (with Z_FIXED and stored among the settings), 15-bit codes, distance 32 768, several blocks
  static const size_t more[] = {0, 1, 2, 63, 64, 65, 257, 258, 259, 288, 289, 4095, 4096, 4097, 65535, 65536};
  for (int kind : {1, 2, 4, 6})
    for (size_t n : more)
      for (int set = 0; set < 4; ++set) {
        Stream s; s.d = make_data(kind, n);
        s.z = set == 0 ? deflate_raw(s.d, 6, Z_DEFAULT_STRATEGY) : set == 1 ? deflate_raw(s.d, 6, Z_FIXED) : set == 2 ? deflate_raw(s.d, 0, Z_DEFAULT_STRATEGY) : deflate_raw(s.d, 9, Z_DEFAULT_STRATEGY, 5);
        valid.push_back(std::move(s));
      }
  for (size_t n : {(size_t)40000, (size_t)65536})
    for (int level : {1, 6, 9}) {
      Stream s; s.d = make_data(7, n); s.z = deflate_raw(s.d, level, Z_DEFAULT_STRATEGY);                                     // distance 32 000, length 258
      if (s.z.size() > 36000) { ++n_bad; fprintf(stderr, "zlib did not find the far matches (n %zu level %d)\n", n, level); }
      valid.push_back(std::move(s));
      Stream t; t.d = make_data(6, n); t.z = deflate_raw(t.d, level, Z_HUFFMAN_ONLY, 3); valid.push_back(std::move(t));     // 15-bit codes, three blocks
    }
  for (size_t dist = 1; dist <= 7; ++dist) {                                                // overlapped copies at every distance 1..7
    Stream s; s.d.resize(3000);
    for (size_t i = 0; i < s.d.size(); ++i) s.d[i] = i < dist ? (uint8_t)('a' + i) : s.d[i - dist];
    s.z = deflate_raw(s.d, 9, Z_DEFAULT_STRATEGY); valid.push_back(std::move(s));
  }
  for (size_t i = 0; i < valid.size(); ++i) {
    if (valid[i].z.size() > dmxzc::kMaxIn) { ++n_bad; fprintf(stderr, "stream %zu is larger than the contract's in_len\n", i); continue; }
    check_valid(valid[i], i < n_shape ? "shape" : "extra");
  }
  // Hand-made dynamic blocks whose distance code is INCOMPLETE: one code of length L.  zlib takes L = 1 only; so must the core.
  // Stream: 'a', <length 3, distance 1>, end of block -> "aaaa"  (the construction of tests/inflate_check.cpp).
  for (int L = 1; L <= 3; ++L) {
    std::vector<uint8_t> z(64, 0);
    size_t bitpos = 0;
    auto put = [&](uint32_t v, int nb) { for (int i = 0; i < nb; ++i, ++bitpos) if ((v >> i) & 1u) z[bitpos >> 3] |= (uint8_t)(1u << (bitpos & 7)); };
    auto code = [&](uint32_t c, int nb) { for (int i = nb - 1; i >= 0; --i, ++bitpos) if ((c >> i) & 1u) z[bitpos >> 3] |= (uint8_t)(1u << (bitpos & 7)); };
    put(1, 1); put(2, 2);
    put(258 - 257, 5); put(0, 5); put(18 - 4, 4);
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int cl_len[19] = {0};
    cl_len[18] = 1; cl_len[1] = 2; cl_len[2] = 2; cl_len[3] = 0;
    if (L == 3) { cl_len[2] = 3; cl_len[3] = 3; }
    for (int i = 0; i < 18; ++i) put((uint32_t)cl_len[order[i]], 3);
    auto zeros = [&](int n) { code(0, 1); put((uint32_t)(n - 11), 7); };
    auto lenv = [&](int v) { if (v == 1) code(2, 2); else if (v == 2) code(L == 3 ? 6 : 3, L == 3 ? 3 : 2); else code(7, 3); };
    zeros(97); lenv(1); zeros(138); zeros(20); lenv(2); lenv(2);
    lenv(L);
    code(0, 1); code(3, 2); code(0, L); code(2, 2);
    const size_t zl = (bitpos + 7) / 8;
    std::vector<uint8_t> mine, zo;
    const bool ok = core_inflate(z.data(), zl, mine, 4) == 0;
    const bool theirs = zlib_inflate(z.data(), zl, zo, 4);
    if (theirs != (L == 1)) { ++n_bad; fprintf(stderr, "hand-made incomplete distance code L=%d: zlib says %d (the test's stream is wrong)\n", L, (int)theirs); }
    if (ok != theirs || (ok && memcmp(mine.data(), "aaaa", 4) != 0)) { ++n_bad; fprintf(stderr, "incomplete distance code L=%d: core %d, zlib %d\n", L, (int)ok, (int)theirs); }
    else ++n_ok;
  }
  // Hand-made: the longest distance DEFLATE can say.  zlib's deflate never emits a distance above 32 768 - 262, so no stream above gets
  // there.  n stored bytes, then a final fixed block <length 258 (symbol 285), distance 32 768 (symbol 29, all 13 extra bits set)>, end of
  // block.  n = 32 768: the copy starts at the member's byte 0; n = 40 000: further in; n = 32 767: one byte too far back — zlib refuses
  // it, and so must the core.  zlib's inflate is the judge of all three.
  size_t n_far = 0;
  for (size_t n : {(size_t)32768, (size_t)40000, (size_t)32767}) {
    std::vector<uint8_t> z(5 + n + 8, 0);
    z[0] = 0; z[1] = (uint8_t)n; z[2] = (uint8_t)(n >> 8); z[3] = (uint8_t)~n; z[4] = (uint8_t)(~n >> 8);
    for (size_t i = 0; i < n; ++i) z[5 + i] = (uint8_t)rnd();
    size_t bitpos = (5 + n) * 8;
    auto put = [&](uint32_t v, int nb) { for (int i = 0; i < nb; ++i, ++bitpos) if ((v >> i) & 1u) z[bitpos >> 3] |= (uint8_t)(1u << (bitpos & 7)); };
    auto code = [&](uint32_t c, int nb) { for (int i = nb - 1; i >= 0; --i, ++bitpos) if ((c >> i) & 1u) z[bitpos >> 3] |= (uint8_t)(1u << (bitpos & 7)); };
    put(1, 1); put(1, 2); code(0xC5, 8); code(29, 5); put(8191, 13); code(0, 7);
    const size_t zl = (bitpos + 7) / 8, want = n + 258;
    std::vector<uint8_t> mine, zo;
    const bool ok = core_inflate(z.data(), zl, mine, want) == 0;
    const bool theirs = zlib_inflate(z.data(), zl, zo, want);
    if (theirs != (n >= 32768)) { ++n_bad; fprintf(stderr, "hand-made distance 32768 after %zu bytes: zlib says %d (the test's stream is wrong)\n", n, (int)theirs); }
    if (ok != theirs || (ok && (mine != zo || memcmp(mine.data() + n, mine.data() + n - 32768, 258) != 0))) { ++n_bad; fprintf(stderr, "distance 32768 after %zu bytes: core %d, zlib %d\n", n, (int)ok, (int)theirs); }
    else { ++n_ok; ++n_far; }
  }
  printf("valid streams ok %zu of %zu, failures %zu\n", n_ok, valid.size() + 3 + n_far, n_bad);

  // ---- damaged: per valid stream four single-bit flips; every fourth stream also a truncation and the sizes n - 1, n + 1, 0
  rng_state = 88172645u;
  for (size_t i = 0; i < valid.size(); ++i) {
    const Stream& s = valid[i];
    if (s.z.empty() || s.z.size() > dmxzc::kMaxIn) continue;
    for (int f = 0; f < 4; ++f) {
      std::vector<uint8_t> bad(s.z);
      bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() & 7));
      check_damaged(bad.data(), bad.size(), s.d.size(), s.d, "flip");
    }
    if (i % 4 == 0) {
      if (s.z.size() > 1) check_damaged(s.z.data(), 1 + rnd() % (s.z.size() - 1), s.d.size(), s.d, "truncated");
      if (s.d.size() > 0) check_damaged(s.z.data(), s.z.size(), s.d.size() - 1, s.d, "n-1");
      if (s.d.size() < 65536) check_damaged(s.z.data(), s.z.size(), s.d.size() + 1, s.d, "n+1");
      if (s.d.size() > 0) check_damaged(s.z.data(), s.z.size(), 0, s.d, "n=0");
    }
  }
  printf("damaged %zu: zlib rejects %zu, zlib accepts with the original bytes %zu, zlib accepts with other bytes %zu; core accepted %zu; failures %zu\n",
         n_dam, n_cls[0], n_cls[1], n_cls[2], n_dam_acc, n_bad);
  if (n_cls[0] * 4 < n_dam || n_cls[2] * 4 < n_dam) { ++n_bad; fprintf(stderr, "the damaged corpus is lopsided: each class must be at least a quarter\n"); }
  // a refused size is a status, not an error
  {
    std::vector<uint8_t> o;
    if (core_inflate((const uint8_t*)"\x03\x00", 2, o, 65537) != dmxzc::ST_LIMIT) { ++n_bad; fprintf(stderr, "out_len 65537 not refused\n"); }
    if (core_inflate((const uint8_t*)"\x03\x00", 2, o, 0) != 0) { ++n_bad; fprintf(stderr, "the empty member is not accepted\n"); }
  }
  int rc = n_bad ? 1 : 0;
  if (argc > 1) rc |= run_file(argv[1], argc > 2 ? argv[2] : nullptr);
  printf("failures %zu\n", n_bad);
  return rc;
}
