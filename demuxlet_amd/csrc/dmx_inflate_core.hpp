// dmx_inflate_core.hpp — the RFC 1951 decoding logic of a BGZF member, written once for the host and the device.
//
// dmx_inflate.hpp is the host's fast path: a 64-bit bit buffer filled by unaligned loads, word-wise match copies that overshoot
// inside an unchecked "fast region".  None of that may run on the device, where the members of a batch lie next to each other in
// one buffer.  This header holds the same decoder with every access checked, parametrised on a policy P that says where the
// tables, the code-length arrays and the output live and how the bulk operations are carried out:
//
//   host   (tests/inflate_core_check.cpp)  heap arrays of exactly the contract's sizes, plain loops: AddressSanitizer sees a stray byte
//   device (dmx_gpu_inflate.hpp)           LDS arrays, one wavefront per member: every lane runs this code with the same values
//                                          (the decoder's state is wave-uniform), and P's bulk operations spread over the lanes
//
// The table entry format, the roots (10 / 8), the caps and the accept / refuse decisions of the canonical-code builder are
// dmx_inflate.hpp's (restated here, since that header is host-only: <zlib.h>, <immintrin.h>, lambdas as leaves).
//
// THE RULES
//   Stores.  Output bytes are written by P::put / P::copy_match / P::copy_in only, and each call is preceded by a check that its
//     byte range lies in [0, out_len) of the member's own output.  Tables and code-length arrays are P's; every index into them
//     is bounded by the constants below (the builder checks `cap` before it opens a second-level table).
//   Loads.  The input is read as aligned 32-bit words of the member's padded staging slot, word index < n_words =
//     (in_len + 8 + 3) / 4, and by P::copy_in for stored blocks, byte range inside [0, in_len).  Bytes at or past in_len read as
//     zero whatever the slot holds (the word is masked), so a member's result does not depend on what follows it.
//   Termination.  `bits_used` = 32 * wpos - bc only grows.  Every trip of every loop either returns, or consumes at least one
//     input bit (a table entry that is not K_BAD has 1 <= bits; a header field, a code length, a repeat count have fixed
//     positive widths), or — a stored block of length 0 — consumes the 3 header bits and the 32 bits of LEN / NLEN.  A trip
//     that needs bits calls need(), which refuses the member as soon as the next word would lie past the slot, that is once
//     the input position passes in_len + 8.  So a member makes at most 8 * (in_len + 12) trips in all, each of bounded work
//     (a table build is at most 2 * 288 symbols and 2048 + 1024 entries; a copy at most 65 535 bytes, and the copied bytes of a
//     member sum to at most out_len, since every copy is checked against the space left).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DMXZC_HD __host__ __device__ inline
#else
#define DMXZC_HD inline
#endif

namespace dmxzc {

enum : uint32_t { K_BAD = 0, K_LIT = 1, K_BASE = 2, K_EOB = 3, K_SUB = 4 };
// bits 0-7 bits to consume (a base: code AND extra bits) | 8-12 extra-bit count (or second-level index width) | 13-15 kind | 16-31 payload
DMXZC_HD uint32_t mk(uint32_t kind, uint32_t nbits, uint32_t extra, uint32_t payload) { return nbits | (extra << 8) | (kind << 13) | (payload << 16); }
DMXZC_HD uint32_t e_bits(uint32_t e) { return e & 0xffu; }
DMXZC_HD uint32_t e_extra(uint32_t e) { return (e >> 8) & 31u; }
DMXZC_HD uint32_t e_kind(uint32_t e) { return (e >> 13) & 7u; }
DMXZC_HD uint32_t e_val(uint32_t e) { return e >> 16; }

constexpr uint32_t kLitRoot = 10, kDistRoot = 8, kClRoot = 7;
constexpr uint32_t kLitCap = 2048, kDistCap = 1024, kClCap = 128;
constexpr uint32_t kLensCap = 286 + 30 + 138;      // a repeat is checked against hlit + hdist before it is written
constexpr uint32_t kSubmaxCap = 1u << kLitRoot;
constexpr uint32_t kCountCap = 48;                 // count[16], next[16], the first pass's copy of next[16]
constexpr uint32_t kMaxOut = 65536, kMaxIn = 65536 + 64;

// status of a member: 0 = accepted; anything else = refused (the values only say why)
enum : int32_t {
  ST_OK = 0, ST_BLOCK_TYPE = 1, ST_INPUT_END = 2, ST_STORED = 3, ST_HEADER = 4, ST_CODE = 5, ST_SYMBOL = 6, ST_OUT_FULL = 7,
  ST_DISTANCE = 8, ST_OUT_SHORT = 9, ST_IN_OVER = 10, ST_LIMIT = 11
};

enum : int { LEAF_CL = 0, LEAF_LIT = 1, LEAF_DIST = 2 };

DMXZC_HD uint32_t bitrev(uint32_t c, uint32_t n) {          // the low n bits of c, reversed (1 <= n <= 15)
  c = ((c >> 1) & 0x55555555u) | ((c & 0x55555555u) << 1);
  c = ((c >> 2) & 0x33333333u) | ((c & 0x33333333u) << 2);
  c = ((c >> 4) & 0x0f0f0f0fu) | ((c & 0x0f0f0f0fu) << 4);
  c = ((c >> 8) & 0x00ff00ffu) | ((c & 0x00ff00ffu) << 8);
  c = (c >> 16) | (c << 16);
  return c >> (32u - n);
}

// RFC 1951 §3.2.5 without tables in memory: length symbols 257..285 and distance symbols 0..29
DMXZC_HD uint32_t leaf(int mode, uint32_t s, uint32_t l) {
  if (mode == LEAF_CL) return mk(K_LIT, l, 0, s);
  if (mode == LEAF_LIT) {
    if (s < 256) return mk(K_LIT, l, 0, s);
    if (s == 256) return mk(K_EOB, l, 0, 0);
    if (s > 285) return mk(K_BAD, l, 0, 0);                  // 286, 287 take part in the fixed code but never occur
    const uint32_t i = s - 257;
    if (i < 8) return mk(K_BASE, l, 0, 3 + i);
    if (i == 28) return mk(K_BASE, l, 0, 258);
    const uint32_t x = (i >> 2) - 1;
    return mk(K_BASE, l + x, x, 3 + ((4 + (i & 3)) << x));
  }
  if (s > 29) return mk(K_BAD, l, 0, 0);
  if (s < 4) return mk(K_BASE, l, 0, s + 1);
  const uint32_t x = (s >> 1) - 1;
  return mk(K_BASE, l + x, x, 1 + ((2 + (s & 1)) << x));
}

// Canonical code of `n` symbols with lengths len[] (0 = unused, every value <= 15) -> lookup table of `root` index bits with
// second-level tables behind it, at most `cap` entries.  False for an over-subscribed or (unless it is the empty or the one-code
// distance case that zlib takes) incomplete code.  The serial part runs with the same values on every lane; P::fill32 / P::fill8
// are the bulk stores.
template <class P>
DMXZC_HD bool build(P& p, const uint8_t* len, uint32_t n, uint32_t root, uint32_t* tab, uint32_t cap, bool allow_incomplete, int mode) {
  uint16_t* const count = p.count; uint16_t* const next = p.count + 16; uint16_t* const nx = p.count + 32;
  p.fill16(count, kCountCap, 0);
  p.sync();
  for (uint32_t i = 0; i < n; ++i) count[len[i] & 15u] = (uint16_t)(count[len[i] & 15u] + 1);
  count[0] = 0;
  int32_t left = 1; uint32_t used = 0;
  bool any_long = false;
  for (uint32_t l = 1; l <= 15; ++l) {
    left = left * 2 - (int32_t)count[l];
    if (left < 0) return false;
    used += count[l];
    if (l > root && count[l]) any_long = true;
  }
  if (left > 0 && !(allow_incomplete && (used == 0 || (used == 1 && count[1] == 1)))) return false;
  uint32_t code = 0;
  for (uint32_t l = 1; l <= 15; ++l) { code = (code + count[l - 1]) << 1; next[l] = (uint16_t)code; nx[l] = (uint16_t)code; }
  const uint32_t rmask = (1u << root) - 1u;
  p.fill32(tab, 0, 1, rmask + 1, 0);
  if (any_long) {                                   // pass 1: the longest code under every root prefix that has long codes
    p.fill8(p.submax, rmask + 1, 0);
    p.sync();
    for (uint32_t s = 0; s < n; ++s) {
      const uint32_t l = len[s] & 15u;
      if (l <= root) { if (l) nx[l] = (uint16_t)(nx[l] + 1); continue; }
      const uint32_t c = nx[l]; nx[l] = (uint16_t)(c + 1);
      const uint32_t q = bitrev(c, l) & rmask;
      if (p.submax[q] < l) p.submax[q] = (uint8_t)l;
    }
  }
  p.sync();
  uint32_t top = rmask + 1;
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = len[s] & 15u;
    if (!l) continue;
    const uint32_t c = next[l]; next[l] = (uint16_t)(c + 1);
    const uint32_t r = bitrev(c, l);
    if (l <= root) {
      p.fill32(tab, r, 1u << l, rmask + 1, leaf(mode, s, l));
    } else {
      const uint32_t q = r & rmask;
      p.sync();
      uint32_t t = tab[q];
      if (e_kind(t) != K_SUB) {
        const uint32_t sb = (uint32_t)p.submax[q] - root;            // 1 .. 15 - root
        if (sb > 15u - root || top + (1u << sb) > cap) return false;
        p.fill32(tab, top, 1, top + (1u << sb), 0);
        t = mk(K_SUB, root, sb, top);
        p.fill32(tab, q, 1, q + 1, t);
        top += 1u << sb;
      }
      const uint32_t sb = e_extra(t), base = e_val(t);
      if (l - root > sb || base + (1u << sb) > cap) return false;    // (cannot happen: submax is the maximum; kept as the bound)
      p.fill32(tab, base + (r >> root), 1u << (l - root), base + (1u << sb), leaf(mode, s, l - root));
    }
  }
  p.sync();
  return true;
}

// the bit reader: aligned words of the padded slot, at least 33 valid bits after need()
struct Bits {
  const uint32_t* w; uint32_t n_words, in_len, wpos; uint64_t bb; uint32_t bc;
};
DMXZC_HD uint32_t word_at(const Bits& b, uint32_t i) {              // i < n_words; bytes at or past in_len are zero
  uint32_t v = b.w[i];
  const uint32_t lo = i * 4u;
  if (lo + 4u > b.in_len) v = lo >= b.in_len ? 0u : (v & (0xffffffffu >> (8u * (lo + 4u - b.in_len))));
  return v;
}
DMXZC_HD bool need(Bits& b) {                                       // false: the input position passed in_len + 8
  while (b.bc <= 32u) {
    if (b.wpos >= b.n_words) return false;
    b.bb |= (uint64_t)word_at(b, b.wpos) << b.bc;
    ++b.wpos; b.bc += 32u;
  }
  return true;
}
DMXZC_HD void drop(Bits& b, uint32_t n) { b.bb >>= n; b.bc -= n; }  // n <= bc (every caller holds >= the bits it drops)
DMXZC_HD uint32_t bits_used(const Bits& b) { return b.wpos * 32u - b.bc; }

// Inflates one raw DEFLATE stream of in_len bytes (slot: n_words = (in_len + 11) / 4 readable aligned words at `in`) into exactly
// out_len bytes of P's output.  Returns a status; ST_OK = the final block ended exactly at out_len, no more than in_len bytes consumed.
template <class P>
DMXZC_HD int32_t inflate_member(P& p, const uint32_t* in, uint32_t in_len, uint32_t out_len) {
  if (in_len > kMaxIn || out_len > kMaxOut) return ST_LIMIT;
  Bits b;
  b.w = in; b.in_len = in_len; b.n_words = (in_len + 8u + 3u) >> 2; b.wpos = 0; b.bb = 0; b.bc = 0;
  uint32_t out = 0;
  for (bool last = false; !last;) {
    if (!need(b)) return ST_INPUT_END;
    last = (b.bb & 1u) != 0;
    const uint32_t type = (uint32_t)(b.bb >> 1) & 3u;
    drop(b, 3);
    if (type == 0) {                                 // stored: to the byte boundary, LEN, ~LEN, bytes
      drop(b, b.bc & 7u);
      if (!need(b)) return ST_INPUT_END;
      const uint32_t n = (uint32_t)b.bb & 0xffffu, nn = (uint32_t)(b.bb >> 16) & 0xffffu;
      drop(b, 32);
      if ((n ^ nn) != 0xffffu) return ST_STORED;
      const uint32_t at = bits_used(b) >> 3;         // a byte boundary
      if (at > in_len || n > in_len - at) return ST_STORED;
      if (n > out_len - out) return ST_OUT_FULL;
      p.copy_in(out, (const uint8_t*)in + at, n);
      out += n;
      const uint32_t to = at + n;                    // <= in_len: word to / 4 lies inside the slot
      b.wpos = to >> 2;
      b.bb = (uint64_t)(word_at(b, b.wpos) >> (8u * (to & 3u)));
      b.bc = 32u - 8u * (to & 3u);
      ++b.wpos;
      continue;
    }
    if (type == 3) return ST_BLOCK_TYPE;
    uint32_t n_lit = 288, n_dist = 32;               // the fixed code (RFC 1951 section 3.2.6), built like any other
    if (type == 1) {
      p.fill8(p.lens, 144, 8); p.fill8(p.lens + 144, 112, 9); p.fill8(p.lens + 256, 24, 7); p.fill8(p.lens + 280, 8, 8);
      p.fill8(p.lens + 288, 32, 5);
      p.sync();
    } else {
      const uint32_t hlit = ((uint32_t)b.bb & 31u) + 257u, hdist = ((uint32_t)(b.bb >> 5) & 31u) + 1u, hclen = ((uint32_t)(b.bb >> 10) & 15u) + 4u;
      drop(b, 14);
      if (hlit > 286 || hdist > 30) return ST_HEADER;
      // the order of the code-length code's lengths (16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15), five bits each
      const uint64_t order_lo = 16ull | (17ull << 5) | (18ull << 10) | (0ull << 15) | (8ull << 20) | (7ull << 25) | (9ull << 30) | (6ull << 35) | (10ull << 40) | (5ull << 45) | (11ull << 50) | (4ull << 55);
      const uint64_t order_hi = 12ull | (3ull << 5) | (13ull << 10) | (2ull << 15) | (14ull << 20) | (1ull << 25) | (15ull << 30);
      p.fill8(p.cl, 19, 0);
      p.sync();
      for (uint32_t i = 0; i < hclen; ++i) {
        if (!need(b)) return ST_INPUT_END;
        const uint32_t sym = i < 12 ? (uint32_t)(order_lo >> (5u * i)) & 31u : (uint32_t)(order_hi >> (5u * (i - 12u))) & 31u;
        p.cl[sym] = (uint8_t)(b.bb & 7u);
        drop(b, 3);
      }
      p.sync();
      if (!build(p, p.cl, 19, kClRoot, p.ct, kClCap, false, LEAF_CL)) return ST_CODE;
      const uint32_t total = hlit + hdist;
      uint32_t i = 0;
      while (i < total) {
        if (!need(b)) return ST_INPUT_END;
        const uint32_t e = p.ct[b.bb & ((1u << kClRoot) - 1u)];
        if (e_kind(e) != K_LIT) return ST_CODE;
        drop(b, e_bits(e));
        const uint32_t s = e_val(e);
        if (s < 16) { p.lens[i++] = (uint8_t)s; continue; }
        uint32_t rep, v = 0;
        if (s == 16) { if (i == 0) return ST_CODE; v = p.lens[i - 1]; rep = 3 + ((uint32_t)b.bb & 3u); drop(b, 2); }
        else if (s == 17) { rep = 3 + ((uint32_t)b.bb & 7u); drop(b, 3); }
        else { rep = 11 + ((uint32_t)b.bb & 127u); drop(b, 7); }
        if (i + rep > total) return ST_CODE;
        p.fill8(p.lens + i, rep, (uint8_t)v);
        p.sync();
        i += rep;
      }
      p.sync();
      if (p.lens[256] == 0) return ST_CODE;
      n_lit = hlit; n_dist = hdist;
    }
    if (!build(p, p.lens, n_lit, kLitRoot, p.lit, kLitCap, false, LEAF_LIT)) return ST_CODE;
    if (!build(p, p.lens + n_lit, n_dist, kDistRoot, p.dist, kDistCap, type == 2, LEAF_DIST)) return ST_CODE;

    // ---- symbols: one per trip; a length / distance pair needs at most 15 + 5 + 15 + 13 = 48 bits, taken in two steps of <= 33
    for (;;) {
      if (!need(b)) return ST_INPUT_END;
      uint32_t e = p.lit[b.bb & ((1u << kLitRoot) - 1u)];
      if (e_kind(e) == K_SUB) { drop(b, kLitRoot); e = p.lit[e_val(e) + ((uint32_t)b.bb & ((1u << e_extra(e)) - 1u))]; }
      const uint32_t k = e_kind(e);
      if (k == K_LIT) {
        if (out >= out_len) return ST_OUT_FULL;
        drop(b, e_bits(e));
        p.put(out, (uint8_t)e_val(e));
        ++out;
        continue;
      }
      if (k == K_EOB) { drop(b, e_bits(e)); break; }
      if (k != K_BASE) return ST_SYMBOL;
      const uint32_t len = e_val(e) + ((uint32_t)(b.bb >> (e_bits(e) - e_extra(e))) & ((1u << e_extra(e)) - 1u));
      drop(b, e_bits(e));
      if (!need(b)) return ST_INPUT_END;
      uint32_t d = p.dist[b.bb & ((1u << kDistRoot) - 1u)];
      if (e_kind(d) == K_SUB) { drop(b, kDistRoot); d = p.dist[e_val(d) + ((uint32_t)b.bb & ((1u << e_extra(d)) - 1u))]; }
      if (e_kind(d) != K_BASE) return ST_SYMBOL;
      const uint32_t dist = e_val(d) + ((uint32_t)(b.bb >> (e_bits(d) - e_extra(d))) & ((1u << e_extra(d)) - 1u));
      drop(b, e_bits(d));
      if (dist > out) return ST_DISTANCE;
      if (len > out_len - out) return ST_OUT_FULL;
      p.copy_match(out, dist, len);
      out += len;
    }
  }
  if (out != out_len) return ST_OUT_SHORT;
  if (((bits_used(b) + 7u) >> 3) > in_len) return ST_IN_OVER;
  return ST_OK;
}

}  // namespace dmxzc
