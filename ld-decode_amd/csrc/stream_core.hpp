// The streamed capture's host bookkeeping (stream.inc is its device half): the chunked
// file reads and the ring arithmetic, with no device call, so tests/san/stream_san.cpp
// drives it on a CPU under ASan / UBSan and ThreadSanitizer.
//
//   file bytes [base_b, fed_b) have been queued into the ring (byte b at b mod R, the ring's
//   first TAIL bytes mirrored after it so a block never wraps); the host promises, through
//   release, that no launch after the call reads bytes below release_b.
//
// Each decision returns what its caller then does on the device.  Methods named *_locked
// are called with `mu` held: the caller's device calls stay under that lock.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <unistd.h>
#include <utility>
#include <vector>

// A chunk's read(2) split over helper threads: the reader's loop is serial (read a chunk,
// queue its copy), and a 60 s u8 step reads 2.4 GB in the ~85 ms the decode takes; with
// four helpers the reads take ~45 ms of it (ldg_stream_stats read_s, profiles/r06_t_*).
struct ReadPool {
  static constexpr int64_t ALIGN = 1 << 16;
  std::mutex m;
  std::condition_variable cv, done_cv;
  std::vector<std::thread> th;
  uint64_t gen = 0;
  int fd = -1, pending = 0;
  uint8_t* dst = nullptr;
  int64_t len = 0, off = 0;
  bool quit = false, err = false;

  void start(int n) {
    for (int i = 0; i < n; i++) th.emplace_back([this, i, n] { run(i, n); });
  }
  void run(int i, int n) {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
      cv.wait(lk, [&] { return quit || gen != seen; });
      if (quit) return;
      seen = gen;
      const int64_t part = ((len + n - 1) / n + ALIGN - 1) / ALIGN * ALIGN;
      const int64_t a = std::min(len, i * part), b = std::min(len, a + part);
      const int f = fd;
      uint8_t* d = dst;
      const int64_t o = off;
      lk.unlock();
      bool ok = true;
      for (int64_t got = a; got < b;) {
        const ssize_t r = pread(f, d + got, (size_t)(b - got), (off_t)(o + got));
        if (r <= 0) { ok = false; break; }
        got += r;
      }
      lk.lock();
      if (!ok) err = true;
      if (--pending == 0) done_cv.notify_all();
    }
  }
  // bytes [o, o + l) of f into d, on every helper; false on a short read or an error
  bool read(int f, uint8_t* d, int64_t l, int64_t o) {
    std::unique_lock<std::mutex> lk(m);
    fd = f; dst = d; len = l; off = o;
    pending = (int)th.size();
    err = false;
    gen++;
    cv.notify_all();
    done_cv.wait(lk, [&] { return pending == 0; });
    return !err;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
      cv.notify_all();
    }
    for (auto& t : th)
      if (t.joinable()) t.join();
    th.clear();
  }
};

struct StreamCore {
  int spg = 1, bpg = 1;                  // samples / bytes per packing group
  int64_t file_bytes = 0, total_nsamp = 0;
  int64_t chunk = 0;                     // reader step (bytes; a multiple of 20: every format's group)
  int64_t R = 0;                         // ring bytes (a multiple of chunk)
  static constexpr int64_t TAIL = 65536; // mirrored head: > one s16 block + a group + 16-B load slack
  static constexpr int NCOPY_MAX = 4;
  int ncopy = NCOPY_MAX;                 // copy streams, chunk c on c % ncopy
  static constexpr int NREL = 256;
  std::deque<std::pair<int64_t, int>> rel;   // (release byte, record), oldest first
  std::vector<int> rel_free;
  std::mutex mu;
  std::condition_variable cv;
  int64_t base_b = 0, fed_b = 0, release_b = 0;
  bool stop = false, failed = false;
  std::string err;
  // statistics (ldg_stream_stats)
  int64_t bytes_read = 0, chunks = 0, launch_waits = 0, seeks = 0;
  double read_s = 0, space_wait_s = 0, launch_wait_s = 0, stage_wait_s = 0;

  int64_t byte_of(int64_t s) const { return s / spg * bpg; }                    // group start
  // the furthest the reader can fill before the next release: whole chunks (file-aligned)
  // whose space lies above the released point
  int64_t reach_b() const { return std::min(file_bytes, (release_b + R) / chunk * chunk); }
  int64_t byte_end(int64_t e) const { return (e + spg - 1) / spg * bpg; }        // through sample e - 1
  int64_t sample_ceil(int64_t b) const { return (b + bpg - 1) / bpg * spg; }     // first whole group at or after b

  static double since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
  }
  static int64_t chunk_for(int64_t ring_bytes) { return std::min<int64_t>(8388600, ring_bytes / 4) / 20 * 20; }
  // the ring a request for ring_bytes gives is the one this core already has
  bool same_ring(int64_t ring_bytes, int nc) const {
    const int64_t c = chunk_for(ring_bytes);
    return c == chunk && ring_bytes / c * c == R && nc == ncopy;
  }
  // chunk and ring size for ring_bytes; false: the ring is too small
  bool configure(int64_t ring_bytes, int nc) {
    ncopy = nc;
    chunk = chunk_for(ring_bytes);
    if (chunk < TAIL) return false;
    R = ring_bytes / chunk * chunk;
    for (int i = 0; i < NREL; i++) rel_free.push_back(i);
    return true;
  }
  void set_file(int64_t bytes, int fmt) {
    spg = fmt == 2 ? 3 : fmt == 3 ? 4 : 1;
    bpg = fmt == 1 ? 2 : fmt == 2 ? 4 : fmt == 3 ? 5 : 1;
    file_bytes = bytes;
    total_nsamp = file_bytes / bpg * spg;
    bytes_read = chunks = launch_waits = seeks = 0;
    read_s = space_wait_s = launch_wait_s = stage_wait_s = 0;
  }
  void request_stop() {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
    cv.notify_all();
  }
  // Start again at the packing group holding `sample`: nothing of the old window is kept.
  // No reader runs and no launch reads the ring.
  void restart(int64_t sample) {
    sample = std::max<int64_t>(0, std::min(sample, total_nsamp));
    base_b = fed_b = release_b = byte_of(sample);
    for (auto& r : rel) rel_free.push_back(r.second);
    rel.clear();
    stop = failed = false;
    err.clear();
  }
  void fail_locked(const std::string& m) {
    failed = true;
    err = m;
    cv.notify_all();
  }
  void fail(const std::string& m) {
    std::lock_guard<std::mutex> lk(mu);
    fail_locked(m);
  }

  // The reader's next chunk: file bytes [fb, fb + len) to ring offset ro, its first `mirror`
  // bytes also to R + ro, on copy stream `copy`, its copy event that of chunk slot `slot`;
  // rec >= 0: the copy stream first waits on that release record's events.
  struct Fill {
    int64_t fb, len, ro, mirror;
    int copy, slot, rec;
  };
  // Blocks until the chunk's space is released; false: stopped, or the file is queued.
  bool next_fill(Fill& f) {
    std::unique_lock<std::mutex> lk(mu);
    const int64_t fb = fed_b;
    if (stop || fb >= file_bytes) return false;
    const int64_t len = std::min(chunk - fb % chunk, file_bytes - fb);
    int rec = -1;
    const int64_t over = fb + len - R;       // this chunk overwrites bytes below `over`
    if (over > base_b) {
      const auto t0 = std::chrono::steady_clock::now();
      cv.wait(lk, [&] { return stop || release_b >= over; });
      space_wait_s += since(t0);
      if (stop) return false;
      // the first release record covering the space; older ones are implied by it
      while (!rel.empty() && rel.front().first < over) {
        rel_free.push_back(rel.front().second);
        rel.pop_front();
      }
      rec = rel.front().second;              // exists: release_b >= over was recorded
    }
    const int64_t ro = fb % R;
    f = {fb, len, ro, ro < TAIL ? std::min(len, TAIL - ro) : 0, (int)((fb / chunk) % ncopy), (int)(ro / chunk), rec};
    return true;
  }
  // the chunk was read from the file; false: stopped, queue nothing
  bool fill_read_locked(const Fill& f, double read, double stage_wait) {
    read_s += read;
    stage_wait_s += stage_wait;
    bytes_read += f.len;
    return !stop;
  }
  // its copies and their events are queued
  void fill_queued_locked(const Fill& f) {
    chunks++;
    fed_b = f.fb + f.len;
    cv.notify_all();
  }

  // The record whose events the caller records on the demod streams before release_commit
  // (a failed record leaves release_b as it was), or -1: nothing to do.
  int release_pick_locked(int64_t b) {
    if (b <= release_b) return -1;
    if (!rel_free.empty()) {
      const int idx = rel_free.back();
      rel_free.pop_back();
      rel.push_back({b, idx});
      return idx;
    }
    rel.back().first = b;                       // out of records: the newest covers more
    return rel.back().second;
  }
  int64_t release_byte(int64_t below_sample) const {
    return byte_of(std::max<int64_t>(0, std::min(below_sample, total_nsamp)));
  }
  void release_commit_locked(int64_t b) {
    release_b = b;
    cv.notify_all();
  }

  // Before a launch whose blocks read samples up to hi: wait (lk holds mu) until the reader
  // has queued them.  OK: the kernels' window is [win_lo, win_hi), and the launch's stream
  // waits on the copy events of chunk slots slot[0 .. nslot).
  enum Status { OK, PAST_RING, TIMEOUT, FAILED };
  struct Launch {
    Status st = OK;
    std::string err;
    int64_t win_lo = 0, win_hi = 0;
    int nslot = 0, slot[NCOPY_MAX] = {};
  };
  Launch prepare_locked(std::unique_lock<std::mutex>& lk, int64_t hi, std::chrono::seconds limit) {
    Launch l;
    auto refused = [&l](Status st, const std::string& m) {
      l.st = st;
      l.err = m;
      return l;
    };
    hi = std::min(hi, total_nsamp);
    int64_t need = byte_end(hi);
    if (need > reach_b())
      return refused(PAST_RING, "stream: a read ends past the ring (release older samples first: ldg_stream_release)");
    if (fed_b < need && !failed) {
      const auto t0 = std::chrono::steady_clock::now();
      launch_waits++;
      // (bounded: the reader reaches `need` unless it failed; a stall is reported, not waited out)
      const bool ok = cv.wait_for(lk, limit, [&] { return failed || fed_b >= need || fed_b >= file_bytes; });
      launch_wait_s += since(t0);
      if (!ok)
        return refused(TIMEOUT, "stream: the reader did not reach byte " + std::to_string(need) + " within " +
                                    std::to_string(limit.count()) + " s");
    }
    if (failed) return refused(FAILED, err);
    need = std::min(need, fed_b);
    l.win_lo = sample_ceil(release_b);
    // the copy of the last chunk the launch reads, on each copy stream (in-order streams:
    // the earlier chunks on it are done with it); chunks wholly released are not read
    const int64_t last = (need - 1) / chunk;
    for (int64_t c = last; c > last - ncopy && c >= 0; c--) {
      if ((c + 1) * chunk <= std::max(base_b, release_b) || c * chunk >= need) continue;
      l.slot[l.nslot++] = (int)((c * chunk % R) / chunk);
    }
    l.win_hi = std::max(l.win_lo, std::min(hi, need / bpg * spg));
    return l;
  }

  void window(int64_t* out4) {
    std::lock_guard<std::mutex> lk(mu);
    out4[0] = sample_ceil(release_b);                         // lowest sample a launch may read
    out4[1] = reach_b() / bpg * spg;                          // ... and the highest block end
    out4[2] = fed_b / bpg * spg;                              // samples queued so far
    out4[3] = total_nsamp;
  }
  int stats(double* out, int n) {
    std::lock_guard<std::mutex> lk(mu);
    const double v[] = {(double)bytes_read, read_s,        (double)chunks, (double)launch_waits,
                        launch_wait_s,      space_wait_s,  (double)seeks,  (double)R,
                        (double)chunk,      stage_wait_s};
    const int m = std::min<int>(n, (int)(sizeof(v) / sizeof(v[0])));
    for (int i = 0; i < m; i++) out[i] = v[i];
    return m;
  }
};
