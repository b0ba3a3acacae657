// Sanitizer driver for the streamed capture's host bookkeeping (test infrastructure, SURVEY
// §5): csrc/stream_core.hpp alone, no libldgpu, no device.  Built twice by the Makefile:
// stream_san (ASan + UBSan) and stream_tsan (ThreadSanitizer).
//
// The model: a host array of R + TAIL bytes is the ring, a reader thread runs stream.inc's
// loop with memcpy for the two device copies, file byte b has the value byte_at(b), and a
// consumer walks the file (release, window, prepare) and checks after every prepare that
// the window's bytes are in the ring, contiguous through the mirrored head.  The consumer
// reads the ring without the core's lock: a refill of space not yet released is a data
// race under ThreadSanitizer.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>

#include "../../ld-decode_amd/csrc/stream_core.hpp"

#ifndef PROG
#define PROG "stream_san"
#endif

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      return false;                                                \
    }                                                              \
  } while (0)

using Core = StreamCore;
static constexpr int64_t TAIL = Core::TAIL;
static const std::chrono::seconds LIMIT(5);

static uint8_t byte_at(int64_t b) { return (uint8_t)(((uint64_t)b * 0x9E3779B97F4A7C15ull) >> 56); }
static std::vector<uint8_t> g_file;          // byte_at(b) for every b a case reads

struct Model {
  Core core;
  std::vector<uint8_t> ring;
  std::thread th;
  int fail_at = -1;                           // the reader fails at this chunk (a read error)
  std::atomic<int> bad{0};                    // the line of a reader-side check that failed
  int64_t exhausted = 0, max_wait_ms = 0;

  bool open(int64_t ring_bytes, int ncopy, int64_t file_bytes, int fmt, int64_t first) {
    if (!core.configure(ring_bytes, ncopy)) return false;
    ring.assign((size_t)(core.R + TAIL), 0xEE);
    core.set_file(file_bytes, fmt);
    start(first);
    return true;
  }
  void start(int64_t sample) {               // as stream_restart
    stop();
    core.restart(sample);
    th = std::thread([this] { reader(); });
  }
  void stop() {
    core.request_stop();
    if (th.joinable()) th.join();
  }
  ~Model() { stop(); }

#define RCHECK(c) \
  if (!(c)) { bad = __LINE__; return core.fail_locked("model: reader check failed"); }
  void reader() {
    Core::Fill f;
    for (int n = 0; core.next_fill(f); n++) {
      if (n == fail_at) return core.fail("stream: read failed in bytes [" + std::to_string(f.fb) + ", " +
                                         std::to_string(f.fb + f.len) + ")");
      std::lock_guard<std::mutex> lk(core.mu);
      if (!core.fill_read_locked(f, 0, 0)) return;
      // a whole file-aligned chunk (or the file's end) into its own slot, nothing past the ring
      RCHECK(f.len > 0 && f.fb == core.fed_b && f.fb + f.len <= core.file_bytes);
      RCHECK(f.fb / core.chunk == (f.fb + f.len - 1) / core.chunk);
      RCHECK((f.fb + f.len) % core.chunk == 0 || f.fb + f.len == core.file_bytes);
      RCHECK(f.ro == f.fb % core.R && f.ro + f.len <= core.R && f.slot == f.ro / core.chunk);
      RCHECK(f.mirror == (f.ro < TAIL ? std::min(f.len, TAIL - f.ro) : 0));
      RCHECK(f.copy == (f.fb / core.chunk) % core.ncopy);
      // what it overwrites is released, and the record it waits on covers that
      const int64_t over = f.fb + f.len - core.R;
      if (over > core.base_b) {
        RCHECK(core.release_b >= over && !core.rel.empty());
        RCHECK(core.rel.front().second == f.rec && core.rel.front().first >= over);
      } else {
        RCHECK(f.rec == -1);
      }
      std::memcpy(ring.data() + f.ro, g_file.data() + f.fb, (size_t)f.len);
      if (f.mirror) std::memcpy(ring.data() + core.R + f.ro, g_file.data() + f.fb, (size_t)f.mirror);
      core.fill_queued_locked(f);
    }
  }

  bool release(int64_t below_sample) {       // as ldg_stream_release
    const int64_t b = core.release_byte(below_sample);
    std::lock_guard<std::mutex> lk(core.mu);
    const int idx = core.release_pick_locked(b);
    if (idx < 0) return true;
    CHECK(idx < Core::NREL && core.rel.back().second == idx && core.rel.back().first == b);
    if (core.rel_free.empty()) exhausted++;
    core.release_commit_locked(b);
    return true;
  }
  Core::Launch prepare(int64_t hi) {         // as stream_prepare
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(core.mu);
    Core::Launch l = core.prepare_locked(lk, hi, LIMIT);
    max_wait_ms = std::max<int64_t>(max_wait_ms, (int64_t)(Core::since(t0) * 1000));
    return l;
  }

  // a successful prepare up to sample hi: its window's bytes are in the ring
  bool check(const Core::Launch& l, int64_t hi) {
    CHECK(l.st == Core::OK && l.err.empty());
    int64_t w[4];
    core.window(w);
    CHECK(l.win_lo == w[0] && l.win_hi == std::max(l.win_lo, hi) && w[3] == core.total_nsamp);
    const int64_t lo_b = core.byte_of(l.win_lo), hi_b = core.byte_end(l.win_hi), R = core.R;
    CHECK(lo_b >= 0 && hi_b <= core.file_bytes && hi_b - lo_b <= R);
    for (int64_t b = lo_b; b < hi_b;) {
      const int64_t n = std::min(hi_b - b, R - b % R);
      CHECK(std::memcmp(ring.data() + b % R, g_file.data() + b, (size_t)n) == 0);
      b += n;
    }
    // runs of TAIL - 16 bytes from the window's start and from around every point where
    // the ring wraps: read straight on from the ring offset, through the mirrored head
    std::vector<int64_t> starts{lo_b};
    for (int64_t m = lo_b / R * R; m < hi_b; m += R)
      for (int64_t k : {(int64_t)1, (int64_t)7, (int64_t)4096, TAIL - 17, TAIL - 16, (int64_t)0})
        if (m - k >= lo_b && m - k < hi_b) starts.push_back(m - k);
    for (int64_t b : starts) {
      const int64_t n = std::min(TAIL - 16, hi_b - b);
      CHECK(b % R + n <= R + TAIL);
      CHECK(std::memcmp(ring.data() + b % R, g_file.data() + b, (size_t)n) == 0);
    }
    // every chunk the window reads is covered by a copy event the launch waits on: the
    // last chunk on the same copy stream at or below the window's last chunk
    const int64_t nslots = R / core.chunk;
    CHECK(l.nslot >= 0 && l.nslot <= core.ncopy);
    for (int i = 0; i < l.nslot; i++) CHECK(l.slot[i] >= 0 && l.slot[i] < nslots);
    if (hi_b > lo_b) {
      const int64_t last = (hi_b - 1) / core.chunk;
      for (int64_t c = lo_b / core.chunk; c <= last; c++) {
        const int64_t cover = last - (last - c) % core.ncopy;
        bool found = false;
        for (int i = 0; i < l.nslot; i++) found |= l.slot[i] == cover % nslots;
        CHECK(found);
      }
    }
    return true;
  }

  // walk from sample pos to sample end (or the file's): release pos - margin every
  // rel_every-th launch, prepare [pos, pos + span) cut at the reach, check; every
  // reach_every-th launch also a prepare up to the whole reach and one a group past it
  bool walk(int64_t pos, int64_t end, int64_t span, int64_t margin, int rel_every, int reach_every) {
    end = std::min(end, core.total_nsamp);
    for (int n = 0; pos < end; n++) {
      if (n % rel_every == 0) CHECK(release(pos - margin));
      int64_t w[4];
      core.window(w);
      CHECK(w[0] <= pos && w[1] <= w[3]);
      const int64_t hi = std::min(std::min(pos + span, w[1]), w[3]);
      CHECK(hi > pos);
      CHECK(check(prepare(hi), hi));
      if (reach_every && n % reach_every == 0) CHECK(reach(w[1]));
      CHECK(!bad);
      pos = hi;
    }
    return true;
  }
  // the reported reach is reachable (the reader fills whole file-aligned chunks: a reach
  // in samples above them is waited for for ever), one group more is refused at once
  bool reach(int64_t reach_s) {
    CHECK(check(prepare(reach_s), reach_s));
    if (reach_s + core.spg <= core.total_nsamp) {
      const int64_t waits = core.launch_waits;   // (only this thread prepares)
      const Core::Launch l = prepare(reach_s + core.spg);
      CHECK(l.st == Core::PAST_RING && core.launch_waits == waits);
      CHECK(l.err == "stream: a read ends past the ring (release older samples first: ldg_stream_release)");
    }
    return true;
  }
  // every release record is in exactly one of the queue and the free list
  bool records() {
    stop();
    std::vector<int> seen(Core::NREL, 0);
    for (auto& r : core.rel) CHECK(r.second >= 0 && r.second < Core::NREL && !seen[r.second]++);
    for (int i : core.rel_free) CHECK(i >= 0 && i < Core::NREL && !seen[i]++);
    CHECK(core.rel.size() + core.rel_free.size() == (size_t)Core::NREL);
    return true;
  }
};

static bool test_configure() {
  Core a, b;
  CHECK(a.configure(262160, 4) && a.chunk == 65540 && a.R == 262160);
  CHECK(!b.configure(262159, 4));                       // chunk 65,520 < TAIL
  CHECK(a.same_ring(262160, 4) && a.same_ring(262160 + 79, 4) && !a.same_ring(262160 + 80, 4));
  CHECK(!a.same_ring(262160, 3) && !a.same_ring(300000, 4) && !a.same_ring(1, 4));
  Core c;
  CHECK(c.configure((int64_t)2 << 30, 2) && c.chunk == 8388600 && c.R == ((int64_t)2 << 30) / 8388600 * 8388600);
  return true;
}

static bool test_sweep() {
  int ncase = 0;
  int64_t max_wait_ms = 0;
  for (int fmt = 0; fmt < 4; fmt++)
    for (int64_t ring : {(int64_t)262160, (int64_t)300000, (int64_t)1 << 20})
      for (int64_t bytes : {(int64_t)0, (int64_t)19, (int64_t)262160, (int64_t)3000017, (int64_t)40 * 65540})
        for (int64_t first : {(int64_t)0, (int64_t)100001})
          for (int wk = 0; wk < 2; wk++) {
            Model m;
            CHECK(m.open(ring, 1 + ncase++ % Core::NCOPY_MAX, bytes, fmt, first));
            const int64_t total = m.core.total_nsamp, from = std::min(first, total);
            CHECK(total == bytes / m.core.bpg * m.core.spg && m.core.base_b == m.core.byte_of(from));
            CHECK(wk ? m.walk(from, total, 16384, 1000, 3, 4) : m.walk(from, total, 50000, 32768, 1, 4));
            CHECK(m.check(m.prepare(total), total));      // the file's end, also of an empty file
            CHECK(m.records() && !m.bad);
            max_wait_ms = std::max(max_wait_ms, m.max_wait_ms);
          }
  CHECK(2 * max_wait_ms < 1000 * LIMIT.count());          // well inside the limit
  std::printf("sweep: %d cases, longest prepare %lld ms\n", ncase, (long long)max_wait_ms);
  return true;
}

static bool test_exhaustion() {
  const int64_t cases[2][3] = {{1, 12000002, 0}, {3, 9000001, 77}};
  for (auto& c : cases) {
    Model m;
    CHECK(m.open((int64_t)4 << 20, 4, c[1], (int)c[0], c[2]));
    CHECK(m.walk(c[2], INT64_MAX, 1000, 1000, 1, 0));
    CHECK(m.exhausted > 0);                                // the queue did run out between refills
    CHECK(m.records() && !m.bad);
    std::printf("exhaustion: fmt %d, %lld releases found no free record\n", (int)c[0], (long long)m.exhausted);
  }
  return true;
}

static bool test_restart_stop() {
  {  // seek backwards and forwards mid-walk
    Model m;
    CHECK(m.open(300000, 4, 3000017, 1, 0));
    CHECK(m.walk(0, 700000, 16384, 1000, 3, 4));
    m.start(12345);
    CHECK(m.core.base_b == 2 * 12345 && m.walk(12345, 400000, 50000, 32768, 1, 4));
    m.start(1000003);
    CHECK(m.walk(1000003, INT64_MAX, 16384, 1000, 3, 4));
    CHECK(m.records() && !m.bad);
  }
  {  // stop with the reader waiting for space: it returns, nothing stays locked, a restart works
    Model m;
    CHECK(m.open(262160, 2, 3000017, 3, 0));
    {
      std::unique_lock<std::mutex> lk(m.core.mu);
      CHECK(m.core.cv.wait_for(lk, LIMIT, [&] { return m.core.fed_b >= m.core.R; }));
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(20));   // ... and is inside its wait
    m.stop();
    CHECK(m.core.fed_b == m.core.R && m.core.mu.try_lock());
    m.core.mu.unlock();
    m.start(4 * 7777);
    CHECK(m.walk(4 * 7777, INT64_MAX, 50000, 32768, 1, 4));
    CHECK(m.records() && !m.bad);
  }
  {  // a reader that failed: prepare returns the failure and the reader's message
    Model m;
    m.fail_at = 2;
    CHECK(m.open(262160, 4, 3000017, 0, 0));
    const Core::Launch l = m.prepare(3 * 65540);
    CHECK(l.st == Core::FAILED && l.err == "stream: read failed in bytes [131080, 196620)");
    const Core::Launch l2 = m.prepare(10);                 // also for bytes that were queued
    CHECK(l2.st == Core::FAILED && l2.err == l.err && !m.bad);
  }
  return true;
}

static bool test_read_pool() {
  const int64_t n = 3 * 1048576 + 12345;
  std::string path = std::string(std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp") + "/stream_san_XXXXXX";
  const int fd = mkstemp(&path[0]);
  CHECK(fd >= 0);
  unlink(path.c_str());
  CHECK(write(fd, g_file.data(), (size_t)n) == (ssize_t)n);
  ReadPool one, four, idle;
  one.start(1);
  four.start(4);
  idle.start(4);
  idle.stop();                                             // started and stopped without a read
  std::vector<uint8_t> a, b;
  for (int64_t len : {(int64_t)1, (int64_t)65535, (int64_t)65536, (int64_t)65537, (int64_t)262147, n})
    for (int64_t off : {(int64_t)0, (int64_t)17, n - len}) {
      if (off + len > n) continue;                         // (the whole file: offset 0 only)
      a.assign((size_t)len + 1, 0xA5);
      b.assign((size_t)len + 1, 0x5A);
      CHECK(four.read(fd, a.data(), len, off) && one.read(fd, b.data(), len, off));
      CHECK(std::memcmp(a.data(), g_file.data() + off, (size_t)len) == 0 && a[(size_t)len] == 0xA5);
      CHECK(std::memcmp(b.data(), g_file.data() + off, (size_t)len) == 0 && b[(size_t)len] == 0x5A);
    }
  a.assign(262147, 0);
  CHECK(!four.read(fd, a.data(), 262147, n - 262147 + 50));   // runs 50 B past the end
  CHECK(!one.read(fd, a.data(), 100, n - 50));
  CHECK(four.read(fd, a.data(), 100, 0));                  // the error does not stick
  one.stop();
  four.stop();                                             // helpers idle
  close(fd);
  return true;
}

int main() {
  g_file.resize(12000002);
  for (size_t b = 0; b < g_file.size(); b++) g_file[b] = byte_at((int64_t)b);
  if (!test_configure() || !test_read_pool() || !test_sweep() || !test_exhaustion() || !test_restart_stop()) return 1;
  std::printf(PROG " ok\n");
  return 0;
}
