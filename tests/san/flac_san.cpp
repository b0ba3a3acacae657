// csrc/flac_plan.hpp (the host logic of the FLAC-compressed captures) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no device, no library.  A valid native file and
// a valid Ogg file (made by tests/flac_ref.py's encoder), then 2,000 seeded mutations of each: byte
// flips, truncations and length fields set to extremes.  Every buffer is allocated at its exact size,
// so a read past the file's end is a report.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../ld-decode_amd/csrc/flac_plan.hpp"

namespace fl = ldg::flac;

static const char* NATIVE_HEX =
    "664c614380000022001000c000000000000009c400f0000000e00acf4e70c513fd712b06dac11800afccfff91008009600fffe5920"
    "fff96008c3800faa02fbb4012cfda80320ff9cfc180190fe0c03840000fc7c01f4fe7003e80064fce08856fff96008c3900ffd1400"
    "0000c6053af9b190886d03a1f0d8647c54cae05987";
static const char* OGG_HEX =
    "4f676753000200000000000000005a1d0000000000001755cf1e01337f464c414301000001664c614300000022001000c000000000000009c400f000"
    "00016c2c7d32b06188288aff4b4e8577d8dff84f676753000000000000000000005a1d00000100000081259ce8042c0b2b1f84000028000000000000"
    "00000000000000000000000000000000000000000000000000000000000000000000fff91008009600fffe5920fff96008c3800faa02fbb4012cfda8"
    "0320ff9cfc180190fe0c03840000fc7c01f4fe7003e80064fce08856fff96008c3900ffd14000000c6053af9b190886d03a1f0d8647c54cae059874f"
    "676753000000000000000000005a1d00000200000083f59e0501fffff96008c3a08b9102e890e890e920ea2fe917e890e903ea11e97ae909e9e7e9b9"
    "e931e9f6e964e92de983e9a1e8a8e890e890e900e9cbe9e2eaa1ea3bea1feacce9eae974e892e890e995e8b9e890e890e92ce890e890e890e890e890"
    "e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890e890"
    "e890e890e890e890e8a9e891e890e890e890e890e890e8ece890e890e930e8a0e890e90fe940e946e9aee9b5ead6eb6eea62e98ee9a9ea69e966e9d4"
    "ea70eb1debfdeb44eb65ec1bebc6eb0ceb00ea05e95dea32ea97eb70ec3ced1eecacec9bece2ec5aed564f676753000100000000000000005a1d0000"
    "030000008323c9340124ec2eecf9ed51ecbded41ed0dedd7ef02ee7fee6dedc2ee36ee8aef59f010f12ff246cf61";

static int fails = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);  \
      fails++;                                                 \
    }                                                          \
  } while (0)

static std::vector<uint8_t> unhex(const char* h) {
  std::vector<uint8_t> out;
  for (; h[0] && h[1]; h += 2) {
    char b[3] = {h[0], h[1], 0};
    out.push_back((uint8_t)std::strtoul(b, nullptr, 16));
  }
  return out;
}

struct Outcome {
  int opened = -1;
  int64_t candidates = 0, headers = 0, packets = 0, kept = 0, nsamples = 0, gaps = 0, broken = 0, lost = 0;
};

// Everything the library's host side does with a file but the device walk: a frame whose header is
// valid is taken as accepted with the longest length the rule allows (R3), so the keeper sees nesting.
static Outcome drive(const std::vector<uint8_t>& file, bool nest = true) {
  // an allocation of exactly the file's size: one byte past it is a report
  std::unique_ptr<uint8_t[]> mem(new uint8_t[file.size() ? file.size() : 1]);
  if (!file.empty()) std::memcpy(mem.get(), file.data(), file.size());
  const uint8_t* b = mem.get();
  const int64_t n = (int64_t)file.size();
  Outcome o;
  fl::Plan P;
  std::string err;
  o.opened = fl::open_file(b, n, &P, &err);
  if (o.opened != 0) {
    CHECK(!err.empty());
    return o;
  }
  const int Bps = P.si.bps / 8;
  CHECK(P.si.channels == 1 && (P.si.bps == 8 || P.si.bps == 16));
  fl::Keeper K;
  if (P.container == fl::NATIVE) {
    CHECK(P.audio_start >= 42 && P.audio_start <= n);
    for (int64_t c = P.audio_start; c + 1 < n; c++) {
      if (b[c] != 0xff || (b[c + 1] & 0xfe) != 0xf8) continue;
      o.candidates++;
      fl::Header h;
      if (!fl::parse_header(b, c, n, P.si.bps, P.si.max_bs, &h)) continue;
      CHECK(h.len >= 6 && h.len <= 16 && h.bs >= 1 && h.bs <= P.si.max_bs && c + h.len <= n);
      o.headers++;
      int64_t len = nest ? fl::frame_bound(h.bs, Bps) : h.len;      // (the valid file's frames do not nest)
      if (len > n - c) len = n - c;
      K.add(c, len, h.variable ? h.number : h.number * P.si.max_bs, h.bs, nullptr);
    }
  } else {
    fl::OggWalker w(b, n);
    fl::Packet pk;
    bool first = true;
    std::vector<uint8_t> buf;
    while (w.next(pk)) {
      int64_t sum = 0;
      for (const fl::Piece& p : pk.pieces) {
        CHECK(p.off >= 0 && p.len > 0 && p.off + p.len <= n);
        sum += p.len;
      }
      CHECK(sum == pk.len && pk.page_off >= 0 && pk.page_off < n && pk.seg >= 0 && pk.seg < 255);
      if (pk.len == 0) continue;
      if (first) {
        first = false;
        continue;
      }
      o.packets++;
      buf.assign((size_t)pk.len, 0);             // exactly the packet's size
      pk.copy_to(b, buf.data(), pk.len);
      if (buf[0] != 0xff) continue;
      o.candidates++;
      fl::Header h;
      if (!fl::parse_header(buf.data(), 0, pk.len, P.si.bps, P.si.max_bs, &h)) continue;
      o.headers++;
      const fl::Where wh{pk.page_off, pk.seg, 0};
      K.add(pk.first_off, pk.len, h.variable ? h.number : h.number * P.si.max_bs, h.bs, &wh);
      // a later walk finds the packet again from where it began
      fl::OggWalker w2(b, n);
      fl::Packet p0, p2;
      CHECK(w2.next(p0));
      CHECK(w2.seek(pk.page_off, pk.seg));
      CHECK(w2.next(p2) && p2.first_off == pk.first_off && p2.len == pk.len);
    }
    o.broken = w.broken;
    o.lost = w.lost;
    CHECK(w.lost >= 0 && w.lost <= n);
  }
  o.kept = K.kept;
  o.nsamples = K.samp_end;
  o.gaps = (int64_t)K.gaps.size() / 2;
  CHECK(K.kept + K.nested + K.misplaced == (int64_t)K.frames.size());
  CHECK((int64_t)K.placed.size() == K.kept);
  int64_t at = 0;
  for (int64_t i : K.placed) {                     // the kept frames ascend and do not overlap
    const fl::Frame& f = K.frames[(size_t)i];
    CHECK(f.state == fl::KEPT && f.pos >= at);
    at = f.pos + f.bs;
  }
  for (int64_t first : {(int64_t)0, K.samp_end / 3, K.samp_end}) {
    int64_t lo, hi;
    K.overlap(first, 100, &lo, &hi);
    CHECK(0 <= lo && lo <= hi && hi <= (int64_t)K.placed.size());
    for (int64_t t = lo; t < hi; t++) {
      const fl::Frame& f = K.frames[(size_t)K.placed[(size_t)t]];
      CHECK(f.pos < first + 100 && f.pos + f.bs > first);
    }
  }
  return o;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

static void mutate(const std::vector<uint8_t>& good, bool ogg) {
  for (int it = 0; it < 2000; it++) {
    std::vector<uint8_t> f = good;
    switch (it % 5) {
      case 0:                                      // byte flips
        for (uint32_t k = 0, m = 1 + rnd() % 4; k < m; k++) f[rnd() % f.size()] ^= (uint8_t)(1u << (rnd() % 8));
        break;
      case 1:                                      // truncation
        f.resize(rnd() % f.size());
        break;
      case 2: {                                    // a length field at an extreme
        const uint8_t ext[] = {0x00, 0x01, 0x7f, 0x80, 0xfe, 0xff};
        if (ogg) {
          // a page's segment count or one of its lacing values
          std::vector<size_t> pages;
          for (size_t i = 0; i + 27 <= f.size(); i++)
            if (!std::memcmp(&f[i], "OggS", 4)) pages.push_back(i);
          const size_t p = pages[rnd() % pages.size()];
          const size_t at = p + 26 + rnd() % 3;
          if (at < f.size()) f[at] = ext[rnd() % 6];
        } else {
          f[5 + rnd() % 3] = ext[rnd() % 6];      // the metadata block's 24-bit length
          if (rnd() & 1) f[4] = ext[rnd() % 6];   // its type and last flag
        }
        break;
      }
      case 3:                                      // bytes overwritten with one value
        for (size_t k = rnd() % f.size(), e = k + 1 + rnd() % 40; k < e && k < f.size(); k++) f[k] = 0xff;
        break;
      default: {                                   // a block size, number or STREAMINFO field at an extreme
        const size_t at = rnd() % f.size();
        f[at] = (rnd() & 1) ? 0xff : 0x00;
        if (at + 1 < f.size() && (rnd() & 1)) f[at + 1] = 0xf9;
        break;
      }
    }
    (void)drive(f);
  }
}

int main() {
  const std::vector<uint8_t> nat = unhex(NATIVE_HEX), ogg = unhex(OGG_HEX);
  Outcome a = drive(nat, false);
  CHECK(a.opened == 0 && a.candidates == 3 && a.headers == 3 && a.kept == 3 && a.nsamples == 224 && a.gaps == 0);
  Outcome b = drive(ogg);
  CHECK(b.opened == 0 && b.candidates == 4 && b.headers == 4 && b.kept == 4 && b.nsamples == 364 && b.gaps == 0);
  CHECK(b.broken == 0 && b.lost == 0 && b.packets == 5);
  CHECK(drive({}).opened != 0);
  CHECK(drive({'I', 'D', '3', 4}).opened != 0);
  CHECK(drive({'f', 'L', 'a', 'C'}).opened != 0);
  CHECK(drive({'O', 'g', 'g', 'S'}).opened != 0);
  mutate(nat, false);
  mutate(ogg, true);
  if (fails) {
    std::printf("flac_san: %d FAIL\n", fails);
    return 1;
  }
  std::printf("flac_san ok\n");
  return 0;
}
