// FLAC-compressed captures (.ldf, .flac, .oga; build-defined): the host logic,
// free of HIP so that it is tested on the CPU (tests/san/flac_san.cpp).  Sniffing and metadata (R0),
// the Ogg page walk into packets, the frame header (R2; shared with the scan kernel of flac.hip) and
// the keep / place bookkeeping (R5, R6).  Every length here is read from an untrusted file: each is
// checked against the file's size before it is used.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define LDG_FLAC_HD __host__ __device__
#else
#define LDG_FLAC_HD
#endif

namespace ldg {
namespace flac {

enum { KEPT = 0, NESTED = 1, MISPLACED = 2 };
enum { NATIVE = 0, OGG = 1 };

struct StreamInfo {
  int32_t min_bs = 0, max_bs = 0, min_frame = 0, max_frame = 0, sample_rate = 0, channels = 0, bps = 0;
  int64_t total = 0;
  uint8_t md5[16] = {};
};

inline void parse_streaminfo(const uint8_t* b, StreamInfo* s) {      // b: 34 bytes
  s->min_bs = b[0] << 8 | b[1];
  s->max_bs = b[2] << 8 | b[3];
  s->min_frame = b[4] << 16 | b[5] << 8 | b[6];
  s->max_frame = b[7] << 16 | b[8] << 8 | b[9];
  uint64_t x = 0;
  for (int i = 0; i < 8; i++) x = x << 8 | b[10 + i];
  s->sample_rate = (int32_t)(x >> 44);
  s->channels = (int32_t)((x >> 41) & 7) + 1;
  s->bps = (int32_t)((x >> 36) & 31) + 1;
  s->total = (int64_t)(x & ((1ull << 36) - 1));
  std::memcpy(s->md5, b + 18, 16);
}

// the longest a frame of bs samples may be (R3): no walk reads past c + frame_bound
LDG_FLAC_HD inline int64_t frame_bound(int64_t bs, int bytes_per_sample) { return 18 + 2 * bs * bytes_per_sample; }

// ---- R2: the frame header ---------------------------------------------------------------------------
struct Header {
  int32_t len, bs, variable, pad_;
  int64_t number;
};

LDG_FLAC_HD inline uint8_t crc8(const uint8_t* b, int64_t n) {
  uint32_t c = 0;
  for (int64_t i = 0; i < n; i++) {
    c ^= b[i];
    for (int k = 0; k < 8; k++) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xff : (c << 1) & 0xff;
  }
  return (uint8_t)c;
}

// The header at b[c ..], none of it at or past b[end].  False: no valid header there.
LDG_FLAC_HD inline bool parse_header(const uint8_t* b, int64_t c, int64_t end, int bps, int max_bs, Header* h) {
  if (c < 0 || c + 5 > end || b[c] != 0xff || (b[c + 1] & 0xfe) != 0xf8) return false;
  const int variable = b[c + 1] & 1;
  const int bsc = b[c + 2] >> 4, src = b[c + 2] & 15;
  const int ch = b[c + 3] >> 4, ssc = (b[c + 3] >> 1) & 7, res = b[c + 3] & 1;
  if (res || bsc == 0 || src == 15 || ch != 0) return false;
  if (ssc != 0 && ssc != (bps == 8 ? 1 : 4)) return false;
  const uint32_t x = b[c + 4];
  int nb;
  uint64_t v;
  if (x < 0x80) {
    nb = 1;
    v = x;
  } else if (x < 0xc0 || x == 0xff) {
    return false;
  } else {
    nb = 2;
    while (x & (0x80u >> nb)) nb++;
    v = x & (0x7fu >> nb);
  }
  if (nb > (variable ? 7 : 6) || c + 4 + nb > end) return false;
  for (int j = 1; j < nb; j++) {
    const uint32_t y = b[c + 4 + j];
    if ((y & 0xc0) != 0x80) return false;
    v = v << 6 | (y & 0x3f);
  }
  int64_t p = c + 4 + nb;
  int32_t bs;
  if (bsc == 1) {
    bs = 192;
  } else if (bsc <= 5) {
    bs = 576 << (bsc - 2);
  } else if (bsc == 6) {
    if (p + 1 > end) return false;
    bs = b[p] + 1;
    p += 1;
  } else if (bsc == 7) {
    if (p + 2 > end) return false;
    bs = (b[p] << 8 | b[p + 1]) + 1;
    p += 2;
  } else {
    bs = 256 << (bsc - 8);
  }
  p += src == 12 ? 1 : (src == 13 || src == 14) ? 2 : 0;
  if (p + 1 > end || bs > max_bs) return false;
  if (crc8(b + c, p - c) != b[p]) return false;
  h->len = (int32_t)(p + 1 - c);
  h->bs = bs;
  h->variable = variable;
  h->pad_ = 0;
  h->number = (int64_t)v;
  return true;
}

// ---- R0: the container ------------------------------------------------------------------------------
struct Piece {
  int64_t off, len;
};

// One packet of the Ogg FLAC stream: its bytes lie in `pieces` of the file; it begins at segment `seg`
// of the page at page_off (where a later walk can start again).
struct Packet {
  int64_t page_off = 0, first_off = 0, len = 0;
  int32_t seg = 0;
  std::vector<Piece> pieces;
  void copy_to(const uint8_t* b, uint8_t* dst, int64_t max_len) const {
    int64_t at = 0;
    for (const Piece& p : pieces) {
      const int64_t l = p.len < max_len - at ? p.len : max_len - at;
      if (l <= 0) break;
      std::memcpy(dst + at, b + p.off, (size_t)l);
      at += l;
    }
  }
};

// The Ogg page walk (R0), one packet a call.  Page CRCs are not verified.  broken: packets dropped
// because their continuation is missing; lost: bytes skipped in searching for a page, the pieces of
// dropped packets and the tails of packets whose heads are missing.
struct OggWalker {
  const uint8_t* b;
  int64_t n;
  int64_t pos = 0;
  bool have_serial = false, has_partial = false, in_page = false, done = false, open_ = false;
  uint32_t serial = 0, last_seq = 0, seq = 0;
  int64_t broken = 0, lost = 0;
  // the page being walked
  int64_t page_off = 0, body = 0, page_end = 0, off = 0, start = 0;
  int nseg = 0, k = 0;
  // the packet being gathered
  std::vector<Piece> cur;
  int64_t cur_page = 0;
  int32_t cur_seg = 0;

  OggWalker(const uint8_t* b_, int64_t n_) : b(b_), n(n_) {}

  static uint32_t u32le(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

  void drop_partial() {
    broken++;
    for (const Piece& p : cur) lost += p.len;
    cur.clear();
    has_partial = false;
  }

  // the next page of this stream; false at the file's end
  bool enter_page() {
    while (!done && pos + 27 <= n) {
      if (std::memcmp(b + pos, "OggS", 4) != 0 || b[pos + 4] != 0) {
        int64_t q = pos + 1;
        while (q + 4 <= n && std::memcmp(b + q, "OggS", 4) != 0) q++;
        if (q + 4 > n) q = n;
        lost += q - pos;
        pos = q;
        continue;
      }
      const int htype = b[pos + 5];
      nseg = b[pos + 26];
      const uint32_t pserial = u32le(b + pos + 14);
      seq = u32le(b + pos + 18);
      body = pos + 27 + nseg;
      int64_t blen = 0;
      if (body <= n)
        for (int i = 0; i < nseg; i++) blen += b[pos + 27 + i];
      if (body + blen > n) {         // a page cut by the file's end is no page
        lost += n - pos;
        pos = n;
        done = true;
        break;
      }
      page_off = pos;
      page_end = body + blen;
      if (!have_serial) {
        if (nseg && blen >= 5 && std::memcmp(b + body, "\x7f" "FLAC", 5) == 0) {
          serial = pserial;
          have_serial = true;
        } else {
          pos = page_end;
          continue;
        }
      }
      if (pserial != serial) {
        pos = page_end;
        continue;
      }
      const bool cont = htype & 1;
      k = 0;
      off = body;
      if (has_partial && !(cont && seq == last_seq + 1u)) drop_partial();
      if (cont && !has_partial) {    // the tail of a packet whose head is not here
        while (k < nseg) {
          const int l = b[page_off + 27 + k];
          lost += l;
          off += l;
          k++;
          if (l < 255) break;
        }
      }
      open_ = has_partial;
      has_partial = false;
      start = off;
      in_page = true;
      return true;
    }
    if (!done) {
      lost += n - pos;
      pos = n;
      done = true;
    }
    if (has_partial) drop_partial();
    return false;
  }

  // the next complete packet (of any kind, possibly empty); false at the end
  bool next(Packet& pk) {
    for (;;) {
      if (!in_page && !enter_page()) return false;
      while (k < nseg) {
        const int l = b[page_off + 27 + k];
        if (!open_) {
          cur_page = page_off;
          cur_seg = k;
        }
        off += l;
        open_ = true;
        k++;
        if (l < 255) {
          if (off > start) cur.push_back({start, off - start});
          start = off;
          open_ = false;
          pk.pieces.swap(cur);
          cur.clear();
          pk.page_off = cur_page;
          pk.seg = cur_seg;
          pk.len = 0;
          for (const Piece& p : pk.pieces) pk.len += p.len;
          pk.first_off = pk.pieces.empty() ? off : pk.pieces[0].off;
          return true;
        }
      }
      if (open_) {
        if (off > start) cur.push_back({start, off - start});
        has_partial = true;
      }
      last_seq = seq;
      pos = page_end;
      in_page = false;
    }
  }

  // start again at segment seg of the page at page_off (a packet's page_off and seg)
  bool seek(int64_t at, int seg) {
    pos = at;
    cur.clear();
    has_partial = in_page = done = open_ = false;
    if (at < 0 || at > n || !enter_page() || page_off != at || seg < 0 || seg > nseg) return false;
    k = seg;
    off = body;
    for (int i = 0; i < seg; i++) off += b[page_off + 27 + i];
    start = off;
    open_ = false;
    return true;
  }
};

struct Plan {
  int container = NATIVE;
  StreamInfo si;
  int64_t audio_start = 0;           // native: the end of the last metadata block
};

// R0 over the whole file b[0, n).  0, or -1 with the reason in err.
inline int open_file(const uint8_t* b, int64_t n, Plan* P, std::string* err) {
  auto refuse = [&](const char* why) {
    *err = why;
    return -1;
  };
  if (n >= 4 && std::memcmp(b, "fLaC", 4) == 0) {
    P->container = NATIVE;
    int64_t pos = 4;
    bool first = true;
    for (;;) {
      if (pos + 4 > n) return refuse("the metadata is cut short");
      const int typ = b[pos] & 0x7f, last = b[pos] >> 7;
      const int64_t len = (int64_t)b[pos + 1] << 16 | b[pos + 2] << 8 | b[pos + 3];
      if (first && (typ != 0 || len != 34)) return refuse("the first metadata block is not STREAMINFO");
      if (typ == 127) return refuse("metadata block type 127");
      if (pos + 4 + len > n) return refuse("the metadata is cut short");
      if (first) parse_streaminfo(b + pos + 4, &P->si);
      first = false;
      pos += 4 + len;
      if (last) break;
    }
    P->audio_start = pos;
  } else if (n >= 4 && std::memcmp(b, "OggS", 4) == 0) {
    P->container = OGG;
    OggWalker w(b, n);
    Packet pk;
    do {
      if (!w.next(pk)) return refuse("no Ogg FLAC stream with a STREAMINFO block");
    } while (pk.len == 0);
    uint8_t head[51];
    if (pk.len < 51) return refuse("no Ogg FLAC stream with a STREAMINFO block");
    pk.copy_to(b, head, 51);
    if (std::memcmp(head + 9, "fLaC", 4) != 0 || (head[13] & 0x7f) != 0 || head[14] != 0 || head[15] != 0 ||
        head[16] != 34)
      return refuse("no Ogg FLAC stream with a STREAMINFO block");
    parse_streaminfo(head + 17, &P->si);
    P->audio_start = 0;
  } else if (n >= 3 && std::memcmp(b, "ID3", 3) == 0) {
    return refuse("the file begins with an ID3 tag; strip it (this project reads fLaC and OggS)");
  } else {
    return refuse("neither fLaC nor OggS");
  }
  if (P->si.channels != 1) return refuse("not one channel");
  if (P->si.bps != 8 && P->si.bps != 16) return refuse("neither 8 nor 16 bits a sample");
  return 0;
}

// ---- R5, R6: keep and place ---------------------------------------------------------------------------
struct Frame {
  int64_t off, nbytes, pos;
  int32_t bs, state;
};

struct Where {                       // Ogg: where a later walk finds the frame's packet
  int64_t page_off;
  int32_t seg, pad_;
};

struct Keeper {
  int64_t byte_end = -1, samp_end = 0, kept_bytes = 0;
  int64_t kept = 0, nested = 0, misplaced = 0, gap_samples = 0;
  std::vector<Frame> frames;         // every accepted frame, in byte order
  std::vector<Where> where;          // (Ogg) of frames[i]
  std::vector<int64_t> placed;       // indices of the kept frames: positions ascending
  std::vector<int64_t> gaps;         // (first, count) pairs

  // the accepted frames arrive in byte order
  void add(int64_t off, int64_t nbytes, int64_t pos, int32_t bs, const Where* w) {
    Frame f{off, nbytes, pos, bs, KEPT};
    if (off < byte_end) {
      f.state = NESTED;
      nested++;
    } else {
      byte_end = off + nbytes;
      if (pos < samp_end) {
        f.state = MISPLACED;
        misplaced++;
      } else {
        if (pos > samp_end) {
          gaps.push_back(samp_end);
          gaps.push_back(pos - samp_end);
          gap_samples += pos - samp_end;
        }
        kept++;
        samp_end = pos + bs;
        kept_bytes += nbytes;
        placed.push_back((int64_t)frames.size());
      }
    }
    frames.push_back(f);
    if (w) where.push_back(*w);
  }

  // the kept frames that overlap samples [first, first + n): indices [lo, hi) of placed
  void overlap(int64_t first, int64_t n, int64_t* lo, int64_t* hi) const {
    int64_t a = 0, b = (int64_t)placed.size();
    while (a < b) {                  // the first frame whose end lies past `first`
      const int64_t m = (a + b) / 2;
      const Frame& f = frames[(size_t)placed[(size_t)m]];
      if (f.pos + f.bs > first) b = m; else a = m + 1;
    }
    *lo = a;
    b = (int64_t)placed.size();
    while (a < b) {                  // the first frame at or past the window's end
      const int64_t m = (a + b) / 2;
      if (frames[(size_t)placed[(size_t)m]].pos >= first + n) b = m; else a = m + 1;
    }
    *hi = a;
  }
};

}  // namespace flac
}  // namespace ldg
