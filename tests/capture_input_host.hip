// tests/capture_input_host.hip — leansdr_amd/csrc/capture_input.h on the host, built and run by tests/test_capture_input_host.py
// (host side only, -ffp-contract=off, AddressSanitizer and UBSan).  No GPU call is made.
//
// For every sample format, 64 bytes of the extreme items at a 16-byte-aligned address: in_unpack of every item of every 16-byte piece
// = in_load of the same item = in_piece either way = float(item − Z)·in_scale as written out here, bit for bit, for in_scale 1 and 1/128.
// Then lsdr_in_describe's table and refusals, and lsdr_in_check_each's refusals with the words the owners' callers look for.
#include <cstdint>
#include <limits>
#include "capture_input.h"

static char g_error[512];
void lsdr_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

static unsigned g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) { ++g_failed; printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same(float2 a, float2 b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y); }

// the expected value of component `j` (0 … 64 / component size − 1) of the buffer, written out: float(item − Z)·in_scale
template <class Expect>
static void check_format(const char *name, int K_, const unsigned char *buf, unsigned flip, float sc, Expect expect) {
  in_dispatch(K_, [&](auto K) {
    constexpr unsigned kB = in_item<K()>::kBytes, kPer = 16u / kB;
    for (unsigned piece = 0; piece < 64u / 16u; ++piece) {
      unsigned ws[4];
      memcpy(ws, buf + 16u * piece, 16);
      float2 wide[kPer], narrow[kPer];
      in_piece<K()>(buf, (size_t)piece * kPer, true, sc, flip, wide);
      in_piece<K()>(buf, (size_t)piece * kPer, false, sc, flip, narrow);
      for (unsigned q = 0; q < kPer; ++q) {
        const unsigned i = piece * kPer + q;
        const float2 u = in_unpack<K()>(ws, q, sc, flip), l = in_load<K()>(buf, i, sc, flip);
        const float2 want = make_float2(expect(2 * i) * sc, expect(2 * i + 1) * sc);
        CHECK(same(u, l), "%s scale %g item %u: unpack (%a, %a), load (%a, %a)", name, sc, i, u.x, u.y, l.x, l.y);
        CHECK(same(l, want), "%s scale %g item %u: load (%a, %a), expected (%a, %a)", name, sc, i, l.x, l.y, want.x, want.y);
        CHECK(same(wide[q], want) && same(narrow[q], want), "%s scale %g item %u: in_piece", name, sc, i);
      }
    }
  });
}

static void check_conversions() {
  static const uint8_t v8[5] = {0, 1, 127, 128, 255};
  static const uint16_t v16[5] = {0x0000, 0x7fff, 0x8000, 0xffff, 0x0001};            // (five: the pairs (re, im) go through all of them)
  static const float v32[5] = {0.0f, -0.0f, 1.5f, -3.25f, 0.75f};
  alignas(16) unsigned char b8[64], b16[64], b32[64];
  for (unsigned j = 0; j < 64; ++j) b8[j] = v8[j % 5];
  for (unsigned j = 0; j < 32; ++j) memcpy(b16 + 2 * j, &v16[j % 5], 2);
  for (unsigned j = 0; j < 16; ++j) memcpy(b32 + 4 * j, &v32[j % 5], 4);
  CHECK(((uintptr_t)b8 & 15u) == 0 && ((uintptr_t)b16 & 15u) == 0 && ((uintptr_t)b32 & 15u) == 0, "the buffers are 16-byte aligned");
  for (float sc : {1.0f, 1.0f / 128.0f}) {
    check_format("cu8", kCapU8, b8, 0u, sc, [&](unsigned j) { return (float)((int)v8[j % 5] - 128); });
    check_format("cs8", kCapS8, b8, 0u, sc, [&](unsigned j) { return (float)(int)(int8_t)v8[j % 5]; });
    check_format("cu16", kCap16, b16, 0x80008000u, sc, [&](unsigned j) { return (float)((int)v16[j % 5] - 32768); });
    check_format("cs16", kCap16, b16, 0u, sc, [&](unsigned j) { return (float)(int)(int16_t)v16[j % 5]; });
    check_format("cf32", kCapF32, b32, 0u, sc, [&](unsigned j) { return v32[j % 5]; });
  }
}

static void check_describe() {
  static const struct { int format, kind; unsigned bytes, flip; } table[5] = {
      {LSDR_IN_CU8, kCapU8, 2, 0u}, {LSDR_IN_CS8, kCapS8, 2, 0u}, {LSDR_IN_CU16, kCap16, 4, 0x80008000u},
      {LSDR_IN_CS16, kCap16, 4, 0u}, {LSDR_IN_CF32, kCapF32, 8, 0u}};
  for (const auto &t : table)
    for (float sc : {0.0f, 1.0f, 1.0f / 128.0f}) {
      lsdr_in_desc d = {-1, 0, 77u, -1.f};
      CHECK(lsdr_in_describe("owner", t.format, sc, &d) == LSDR_OK, "format %d scale %g", t.format, sc);
      CHECK(d.kind == t.kind && d.item_bytes == t.bytes && d.in_flip == t.flip, "format %d: kind %d, %u bytes, flip %#x", t.format, d.kind, d.item_bytes, d.in_flip);
      CHECK(bits(d.in_scale) == bits(sc == 0.0f ? 1.0f : sc), "format %d scale %g gives %g", t.format, sc, d.in_scale);
    }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (int format : {-1, 5}) {
    lsdr_in_desc d = {-1, 0, 77u, -1.f};
    g_error[0] = 0;
    CHECK(lsdr_in_describe("owner", format, 0.0f, &d) == LSDR_E_ARG && d.kind == -1, "format %d is refused, nothing written", format);
    CHECK(strstr(g_error, "owner") && strstr(g_error, "in_format"), "format %d: \"%s\"", format, g_error);
  }
  for (float sc : {-1.0f, nan, inf, -inf}) {
    lsdr_in_desc d = {-1, 0, 77u, -1.f};
    g_error[0] = 0;
    CHECK(lsdr_in_describe("owner", LSDR_IN_CS16, sc, &d) == LSDR_E_ARG && d.kind == -1, "scale %g is refused, nothing written", sc);
    CHECK(strstr(g_error, "owner") && strstr(g_error, "in_scale"), "scale %g: \"%s\"", sc, g_error);
  }
}

static void check_each() {
  alignas(16) static unsigned char mem[64];
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  auto refused = [&](const char *what, const char *word, const void *p1, size_t n1, float tune1, int reserved1, unsigned item_bytes, bool as_each) {
    const void *iq[2] = {mem, p1};
    lsdr_capture_each each[2];
    memset(each, 0, sizeof each);
    each[0].n_samples = 4; each[1].n_samples = n1; each[1].tune = tune1; each[1].reserved[4] = reserved1;
    const size_t n[2] = {4, n1};
    const float tune[2] = {0.f, tune1};
    g_error[0] = 0;
    const int rc = as_each ? lsdr_in_check_each("owner", "the word", 2, iq, each, nullptr, nullptr, 8, item_bytes)
                           : lsdr_in_check_each("owner", "the word", 2, iq, nullptr, n, tune, 8, item_bytes);
    if (!word) { CHECK(rc == LSDR_OK, "%s: \"%s\"", what, g_error); return; }
    CHECK(rc == LSDR_E_ARG, "%s is refused", what);
    CHECK(strstr(g_error, "owner") && strstr(g_error, "capture 1") && strstr(g_error, word), "%s: \"%s\"", what, g_error);
  };
  for (bool as_each : {true, false}) {
    refused("a good batch", nullptr, mem + 8, 8, -0.25f, 0, 8, as_each);
    refused("no samples and no pointer", nullptr, nullptr, 0, 0.f, 0, 8, as_each);
    refused("n_samples > max_samples", "max_samples", mem, 9, 0.f, 0, 2, as_each);
    for (float t : {nan, inf, 0.5f, -0.5f, 0.75f}) refused("a tune outside (-0.5, 0.5)", "the word", mem, 8, t, 0, 2, as_each);
    refused("samples and no pointer", "no pointer", nullptr, 1, 0.f, 0, 2, as_each);
    refused("a pointer at 1 of 2 bytes", "aligned", mem + 1, 8, 0.f, 0, 2, as_each);
    refused("a pointer at 2 of 4 bytes", "aligned", mem + 2, 8, 0.f, 0, 4, as_each);
    refused("a pointer at 4 of 8 bytes", "aligned", mem + 4, 8, 0.f, 0, 8, as_each);
  }
  refused("nonzero reserved", "reserved", mem, 8, 0.f, 1, 2, true);
  // lengths alone (no tune to check): the estimator's call
  const void *iq[1] = {mem};
  const size_t n[1] = {1u << 20};
  CHECK(lsdr_in_check_each("owner", "tune", 1, iq, nullptr, n, nullptr, ~(size_t)0, 2) == LSDR_OK, "lengths alone: \"%s\"", g_error);
}

int main() {
  check_conversions();
  check_describe();
  check_each();
  printf("%u checks, %u failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
