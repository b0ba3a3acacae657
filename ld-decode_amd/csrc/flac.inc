// Host side of the FLAC-compressed captures (flac.hip, flac_plan.hpp; build-defined, DESIGN.md section
// 7g): ldg_flac_* of include/ldgpu.h.  Unity-built after abi.inc, whose launch and error helpers it
// uses.  The file is mapped; its bytes reach the device through one pinned staging buffer.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

struct ldg_flac_state {
  int fd = -1;
  const uint8_t* map = nullptr;
  int64_t n = 0;
  ldg::flac::Plan plan;
  bool indexed = false;
  ldg::flac::Keeper keep;
  ldg_flac_counters cnt = {};
  hipStream_t st = nullptr;
  int64_t buf_bytes = 0;             // bytes of the file a launch sees (h_buf and d_buf hold 64 more)
  uint8_t *h_buf = nullptr, *d_buf = nullptr;
  ldg::flac::Job* d_jobs = nullptr;
  ldg::flac::Res* d_res = nullptr;
  ldg::flac::PlaceRec* d_recs = nullptr;
  uint32_t *d_cand = nullptr, *d_counts = nullptr;
  int32_t* d_scratch = nullptr;      // [scratch_bs][nslots]: the decode slots' samples
  int nslots = 0, scratch_bs = 0;
  uint8_t* d_tmp = nullptr;          // ldg_flac_read into host memory
  int64_t tmp_bytes = 0;
};

namespace {

constexpr int FLAC_JOB_CAP = 1 << 16;        // candidates a walk launch takes
constexpr uint32_t FLAC_CAND_CAP = 1 << 18;  // valid headers a scan launch can list
constexpr int64_t FLAC_CHUNK = 64ll << 20;   // ldg_flac_index's default chunk
constexpr int64_t FLAC_SCRATCH = 256ll << 20;

void flac_unmap(ldg_flac_state* S) {
  if (S->map) (void)munmap((void*)S->map, (size_t)S->n);
  if (S->fd >= 0) (void)close(S->fd);
  S->map = nullptr;
  S->fd = -1;
  S->n = 0;
  S->indexed = false;
  S->keep = ldg::flac::Keeper();
  S->cnt = ldg_flac_counters{};
}

int flac_state(ldg_ctx* ctx, const char* fn, bool need_index, ldg_flac_state** out) {
  ldg_flac_state* S = ctx->flac;
  if (!S || !S->map) {
    ctx->err = std::string(fn) + ": no file is open (ldg_flac_open)";
    return LDG_ESTATE;
  }
  if (need_index && !S->indexed) {
    ctx->err = std::string(fn) + ": the file has no index yet (ldg_flac_index)";
    return LDG_ESTATE;
  }
  *out = S;
  return LDG_OK;
}

// staging for launches over `bytes` of the file, and the small per-launch arrays
int flac_buffers(ldg_ctx* ctx, ldg_flac_state* S, int64_t bytes) {
  int rc;
  if (!S->st && hipStreamCreateWithFlags(&S->st, hipStreamNonBlocking) != hipSuccess) {
    S->st = nullptr;
    ctx->err = "flac: hipStreamCreate failed";
    return LDG_EDEVICE;
  }
  if (!S->d_jobs) {
    if ((rc = dmalloc(ctx, &S->d_jobs, (size_t)FLAC_JOB_CAP))) return rc;
    if ((rc = dmalloc(ctx, &S->d_res, (size_t)FLAC_JOB_CAP))) return rc;
    if ((rc = dmalloc(ctx, &S->d_recs, (size_t)FLAC_JOB_CAP))) return rc;
    if ((rc = dmalloc(ctx, &S->d_cand, (size_t)FLAC_CAND_CAP))) return rc;
    if ((rc = dmalloc(ctx, &S->d_counts, (size_t)ldg::flac::SCAN_COUNTS))) return rc;
  }
  if (bytes > S->buf_bytes) {
    if (S->h_buf) (void)hipHostFree(S->h_buf);
    dfree(S->d_buf);
    S->h_buf = S->d_buf = nullptr;
    S->buf_bytes = 0;
    if (hipHostMalloc((void**)&S->h_buf, (size_t)bytes + 64) != hipSuccess) {
      S->h_buf = nullptr;
      ctx->err = "flac: hipHostMalloc of the staging buffer failed";
      return LDG_ENOMEM;
    }
    if ((rc = dmalloc(ctx, &S->d_buf, (size_t)bytes + 64))) return rc;
    S->buf_bytes = bytes;
  }
  return LDG_OK;
}

// the first `len` staged bytes to the device, zeros behind them to the next words
int flac_upload(ldg_ctx* ctx, ldg_flac_state* S, int64_t len) {
  std::memset(S->h_buf + len, 0, 64);
  LDG_TRY(hipMemcpyAsync(S->d_buf, S->h_buf, (size_t)len + 64, hipMemcpyHostToDevice, S->st));
  return LDG_OK;
}

// walk jobs[0, m) over the staged bytes (len of them); res receives the verdicts
template <bool EMIT>
int flac_walk(ldg_ctx* ctx, ldg_flac_state* S, const ldg::flac::Job* jobs, int m, int64_t len, ldg::flac::Res* res) {
  if (m == 0) return LDG_OK;
  int rc;
  LDG_TRY(hipMemcpyAsync(S->d_jobs, jobs, (size_t)m * sizeof(ldg::flac::Job), hipMemcpyHostToDevice, S->st));
  LDG_LAUNCH_ON(S->st, EMIT ? "flac_decode" : "flac_walk", ldg::flac::ldg_k_flac_walk<EMIT>, (unsigned)((m + 63) / 64), 64,
                (const uint64_t*)S->d_buf, (len + 64) / 8, S->d_jobs, m, S->plan.si.bps, S->d_res, S->d_scratch, S->nslots);
  if ((rc = check_launch(ctx, "ldg_k_flac_walk"))) return rc;
  LDG_TRY(hipMemcpyAsync(res, S->d_res, (size_t)m * sizeof(ldg::flac::Res), hipMemcpyDeviceToHost, S->st));
  LDG_TRY(hipStreamSynchronize(S->st));
  return LDG_OK;
}

// the valid headers of staged bytes [lo, hi) (none reading at or past len), ascending, added to offs
int flac_scan(ldg_ctx* ctx, ldg_flac_state* S, int64_t lo, int64_t hi, int64_t len, std::vector<uint32_t>* offs) {
  if (hi <= lo) return LDG_OK;
  int rc;
  uint32_t counts[ldg::flac::SCAN_COUNTS];
  LDG_TRY(hipMemsetAsync(S->d_counts, 0, sizeof(counts), S->st));
  LDG_LAUNCH_ON(S->st, "flac_scan", ldg::flac::ldg_k_flac_scan, (unsigned)((hi - lo + 255) / 256), 256, S->d_buf, lo, hi, len,
                S->plan.si.bps, S->plan.si.max_bs, S->d_cand, FLAC_CAND_CAP, S->d_counts);
  if ((rc = check_launch(ctx, "ldg_k_flac_scan"))) return rc;
  LDG_TRY(hipMemcpyAsync(counts, S->d_counts, sizeof(counts), hipMemcpyDeviceToHost, S->st));
  LDG_TRY(hipStreamSynchronize(S->st));
  if (counts[1] > FLAC_CAND_CAP) {   // more than the list holds: the two halves on their own
    const int64_t mid = lo + (hi - lo) / 2;
    if ((rc = flac_scan(ctx, S, lo, mid, len, offs))) return rc;
    return flac_scan(ctx, S, mid, hi, len, offs);
  }
  S->cnt.candidates += counts[0];
  const size_t at = offs->size();
  offs->resize(at + counts[1]);
  if (counts[1]) {
    LDG_TRY(hipMemcpyAsync(offs->data() + at, S->d_cand, counts[1] * sizeof(uint32_t), hipMemcpyDeviceToHost, S->st));
    LDG_TRY(hipStreamSynchronize(S->st));
    std::sort(offs->begin() + (long)at, offs->end());
  }
  return LDG_OK;
}

struct FlacPending {                 // a job's frame, for the keeper
  int64_t off, pos;
  int32_t bs;
  ldg::flac::Where where;
};

// walk the jobs and hand the accepted frames, which are in byte order, to the keeper
int flac_index_jobs(ldg_ctx* ctx, ldg_flac_state* S, std::vector<ldg::flac::Job>& jobs, std::vector<FlacPending>& pend,
                    int64_t len, bool ogg) {
  std::vector<ldg::flac::Res> res((size_t)FLAC_JOB_CAP);
  for (size_t j0 = 0; j0 < jobs.size(); j0 += FLAC_JOB_CAP) {
    const int m = (int)std::min<size_t>(FLAC_JOB_CAP, jobs.size() - j0);
    if (int rc = flac_walk<false>(ctx, S, jobs.data() + j0, m, len, res.data())) return rc;
    for (int j = 0; j < m; j++) {
      const FlacPending& P = pend[j0 + j];
      const int st = res[j].state;
      if (st >= ldg::flac::ST_PARSED) S->cnt.parsed++;
      if (st == ldg::flac::ST_RANGE) S->cnt.range++;
      if (st != ldg::flac::ST_ACCEPT) continue;
      S->cnt.accepted++;
      S->keep.add(P.off, res[j].nbytes, P.pos, P.bs, ogg ? &P.where : nullptr);
    }
  }
  jobs.clear();
  pend.clear();
  return LDG_OK;
}

// a valid header's frame: its position, or the refusal of R2
int flac_position(ldg_ctx* ctx, const ldg_flac_state* S, const ldg::flac::Header& h, int64_t* pos) {
  const ldg::flac::StreamInfo& si = S->plan.si;
  if (!h.variable && si.min_bs != si.max_bs) {
    ctx->err = "ldg_flac_index: a fixed-block-size frame in a stream whose STREAMINFO block sizes differ";
    return LDG_EINVAL;
  }
  *pos = h.variable ? h.number : h.number * si.max_bs;
  return LDG_OK;
}

}  // namespace

static void flac_free(ldg_ctx* ctx) {
  ldg_flac_state* S = ctx->flac;
  if (!S) return;
  if (S->st) {
    (void)hipStreamSynchronize(S->st);
    (void)hipStreamDestroy(S->st);
  }
  flac_unmap(S);
  if (S->h_buf) (void)hipHostFree(S->h_buf);
  for (void* p : {(void*)S->d_buf, (void*)S->d_jobs, (void*)S->d_res, (void*)S->d_recs, (void*)S->d_cand,
                  (void*)S->d_counts, (void*)S->d_scratch, (void*)S->d_tmp})
    dfree(p);
  delete S;
  ctx->flac = nullptr;
}

int ldg_flac_open(ldg_ctx* ctx, const char* path, ldg_flac_info* info) {
  if (!ctx) return LDG_EINVAL;
  if (!path || !info) {
    ctx->err = "ldg_flac_open: path and info must not be NULL";
    return LDG_EINVAL;
  }
  if (!ctx->flac) ctx->flac = new (std::nothrow) ldg_flac_state();
  ldg_flac_state* S = ctx->flac;
  if (!S) {
    ctx->err = "ldg_flac_open: out of memory";
    return LDG_ENOMEM;
  }
  flac_unmap(S);
  auto refuse = [&](const std::string& why) {
    flac_unmap(S);
    ctx->err = std::string("ldg_flac_open: ") + path + ": " + why;
    return LDG_EINVAL;
  };
  S->fd = open(path, O_RDONLY);
  struct stat sb;
  if (S->fd < 0 || fstat(S->fd, &sb) != 0) return refuse("cannot open the file");
  if (sb.st_size < 4) return refuse("neither fLaC nor OggS");
  void* m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, S->fd, 0);
  if (m == MAP_FAILED) return refuse("cannot map the file");
  S->map = (const uint8_t*)m;
  S->n = (int64_t)sb.st_size;
  S->plan = ldg::flac::Plan();
  std::string why;
  if (ldg::flac::open_file(S->map, S->n, &S->plan, &why) != 0) return refuse(why);
  const ldg::flac::StreamInfo& si = S->plan.si;
  *info = ldg_flac_info{};
  info->container = S->plan.container;
  info->fmt = si.bps == 16 ? LDG_FMT_S16 : LDG_FMT_U8;
  info->bps = si.bps;
  info->channels = si.channels;
  info->sample_rate = si.sample_rate;
  info->min_block = si.min_bs;
  info->max_block = si.max_bs;
  info->total_samples = si.total;
  info->file_bytes = S->n;
  info->audio_offset = S->plan.audio_start;
  std::memcpy(info->md5, si.md5, 16);
  return LDG_OK;
}

int ldg_flac_index(ldg_ctx* ctx, int64_t chunk_bytes, ldg_flac_counters* out) {
  if (!ctx) return LDG_EINVAL;
  ldg_flac_state* S;
  int rc;
  if ((rc = flac_state(ctx, "ldg_flac_index", false, &S))) return rc;
  if (chunk_bytes < 0 || !out) {
    ctx->err = "ldg_flac_index: chunk_bytes must be >= 0 and out not NULL";
    return LDG_EINVAL;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  namespace fl = ldg::flac;
  const fl::StreamInfo& si = S->plan.si;
  const int Bps = si.bps / 8;
  const int64_t bound = fl::frame_bound(si.max_bs, Bps);
  int64_t chunk = chunk_bytes ? chunk_bytes : FLAC_CHUNK;
  chunk = std::min<int64_t>(std::max<int64_t>(chunk, 256), 1ll << 30);
  chunk = (chunk + 255) / 256 * 256;
  if ((rc = flac_buffers(ctx, S, chunk + bound))) return rc;
  S->indexed = false;
  S->keep = fl::Keeper();
  S->cnt = ldg_flac_counters{};
  std::vector<fl::Job> jobs;
  std::vector<FlacPending> pend;
  int64_t region_bytes = 0, lost0 = 0;
  if (S->plan.container == fl::NATIVE) {
    std::vector<uint32_t> offs;
    region_bytes = S->n - S->plan.audio_start;
    for (int64_t a = S->plan.audio_start; a < S->n; a += chunk) {
      const int64_t len = std::min(chunk + bound, S->n - a), scan_hi = std::min(chunk, S->n - a);
      std::memcpy(S->h_buf, S->map + a, (size_t)len);
      if ((rc = flac_upload(ctx, S, len))) return rc;
      offs.clear();
      if ((rc = flac_scan(ctx, S, 0, scan_hi, len, &offs))) return rc;
      for (uint32_t c : offs) {
        fl::Header h;
        if (!fl::parse_header(S->h_buf, c, len, si.bps, si.max_bs, &h)) continue;
        int64_t pos;
        if ((rc = flac_position(ctx, S, h, &pos))) return rc;
        S->cnt.header_ok++;
        jobs.push_back({(int64_t)c, std::min<int64_t>(c + fl::frame_bound(h.bs, Bps), len), h.bs, h.len, 0, 0});
        pend.push_back({a + c, pos, h.bs, {0, 0, 0}});
      }
      if ((rc = flac_index_jobs(ctx, S, jobs, pend, len, false))) return rc;
    }
  } else {
    fl::OggWalker w(S->map, S->n);
    fl::Packet pk;
    bool first = true, more = true, held = false;
    while (more) {
      int64_t used = 0;
      while (held || (more = w.next(pk))) {
        if (!held) {
          if (pk.len == 0) continue;
          if (first) {               // the mapping's own packet
            first = false;
            continue;
          }
          if (S->map[pk.first_off] != 0xff) continue;      // a header packet, whatever the stated count
          S->cnt.candidates++;
          region_bytes += pk.len;
        }
        uint8_t head[16];
        const int64_t hl = std::min<int64_t>(pk.len, 16);
        pk.copy_to(S->map, head, hl);
        fl::Header h;
        if (!fl::parse_header(head, 0, hl, si.bps, si.max_bs, &h)) {
          held = false;
          continue;
        }
        if (!held) {
          int64_t pos;
          if ((rc = flac_position(ctx, S, h, &pos))) return rc;
          S->cnt.header_ok++;
          if (pk.len > fl::frame_bound(h.bs, Bps)) continue;      // cannot end at the packet's end
        }
        if (used + pk.len > chunk + bound || (int)jobs.size() == FLAC_JOB_CAP) {
          held = true;               // this packet opens the next launch
          break;
        }
        held = false;
        pk.copy_to(S->map, S->h_buf + used, pk.len);
        jobs.push_back({used, used + pk.len, h.bs, h.len, 1, 0});
        pend.push_back({pk.first_off, h.variable ? h.number : h.number * si.max_bs, h.bs, {pk.page_off, pk.seg, 0}});
        used += pk.len;
      }
      if (!jobs.empty()) {
        if ((rc = flac_upload(ctx, S, used))) return rc;
        if ((rc = flac_index_jobs(ctx, S, jobs, pend, used, true))) return rc;
      }
    }
    S->cnt.ogg_broken = w.broken;
    lost0 = w.lost;
  }
  const fl::Keeper& K = S->keep;
  S->cnt.kept = K.kept;
  S->cnt.nested = K.nested;
  S->cnt.misplaced = K.misplaced;
  S->cnt.gaps = (int64_t)K.gaps.size() / 2;
  S->cnt.gap_samples = K.gap_samples;
  S->cnt.lost_bytes = lost0 + region_bytes - K.kept_bytes;
  S->cnt.nsamples = K.samp_end;
  S->cnt.frames = (int64_t)K.frames.size();
  S->indexed = true;
  *out = S->cnt;
  prof_collect(ctx);
  return LDG_OK;
}

int ldg_flac_frames(ldg_ctx* ctx, ldg_flac_frame* frames, int64_t cap_frames, int64_t* gaps, int64_t cap_gaps) {
  if (!ctx) return LDG_EINVAL;
  ldg_flac_state* S;
  if (int rc = flac_state(ctx, "ldg_flac_frames", true, &S)) return rc;
  if (cap_frames < 0 || cap_gaps < 0 || (cap_frames && !frames) || (cap_gaps && !gaps)) {
    ctx->err = "ldg_flac_frames: a capacity without its array";
    return LDG_EINVAL;
  }
  const int64_t nf = std::min<int64_t>(cap_frames, (int64_t)S->keep.frames.size());
  if (nf) std::memcpy(frames, S->keep.frames.data(), (size_t)nf * sizeof(ldg_flac_frame));
  const int64_t ng = std::min<int64_t>(cap_gaps, (int64_t)S->keep.gaps.size() / 2);
  if (ng) std::memcpy(gaps, S->keep.gaps.data(), (size_t)ng * 2 * sizeof(int64_t));
  return LDG_OK;
}

// samples [first, first + n) into device memory d
static int flac_decode_to(ldg_ctx* ctx, ldg_flac_state* S, int64_t first, int64_t n, void* d) {
  namespace fl = ldg::flac;
  const fl::StreamInfo& si = S->plan.si;
  const int Bps = si.bps / 8;
  int rc;
  if ((rc = flac_buffers(ctx, S, std::max<int64_t>(S->buf_bytes, fl::frame_bound(si.max_bs, Bps))))) return rc;
  if (!S->d_scratch || S->scratch_bs < si.max_bs) {      // (the state outlives a file: sized for this one's blocks)
    dfree(S->d_scratch);
    S->d_scratch = nullptr;
    S->nslots = S->scratch_bs = 0;
    const int rows = std::max(si.max_bs, 1);
    int64_t slots = FLAC_SCRATCH / (4 * (int64_t)rows) / 64 * 64;
    slots = std::min<int64_t>(std::max<int64_t>(slots, 64), 8192);
    if ((rc = dmalloc(ctx, &S->d_scratch, (size_t)slots * (size_t)rows))) return rc;
    S->nslots = (int)slots;
    S->scratch_bs = rows;
  }
  LDG_TRY(hipMemsetAsync(d, si.bps == 8 ? 0x80 : 0, (size_t)n * Bps, S->st));
  int64_t lo, hi;
  S->keep.overlap(first, n, &lo, &hi);
  const bool ogg = S->plan.container == fl::OGG;
  fl::OggWalker w(S->map, S->n);
  fl::Packet pk;
  w.have_serial = false;
  bool walking = false;
  std::vector<fl::Job> jobs;
  std::vector<fl::PlaceRec> recs;
  std::vector<fl::Res> res((size_t)S->nslots);
  auto changed = [&]() {
    ctx->err = "ldg_flac_read: the file no longer holds the frames of its index";
    return LDG_ESTATE;
  };
  for (int64_t t = lo; t < hi;) {
    jobs.clear();
    recs.clear();
    int64_t used = 0;
    int max_bs = 0;
    const int64_t base = S->keep.frames[(size_t)S->keep.placed[(size_t)t]].off;
    for (; t < hi && (int)jobs.size() < S->nslots; t++) {
      const size_t fi = (size_t)S->keep.placed[(size_t)t];
      const fl::Frame& f = S->keep.frames[fi];
      int64_t at;
      if (ogg) {
        if (used + f.nbytes > S->buf_bytes) break;
        if (!walking) {
          // the stream's serial, then the packet's own page
          fl::Packet first_pk;
          if (!w.next(first_pk) || !w.seek(S->keep.where[fi].page_off, S->keep.where[fi].seg)) return changed();
          walking = true;
        }
        do {
          if (!w.next(pk) || (pk.len && pk.first_off > f.off)) return changed();
        } while (pk.len == 0 || pk.first_off != f.off);
        if (pk.len != f.nbytes) return changed();
        at = used;
        pk.copy_to(S->map, S->h_buf + at, pk.len);
        used += pk.len;
      } else {
        at = f.off - base;
        if (at + f.nbytes > S->buf_bytes) break;
        if (f.off < 0 || f.off + f.nbytes > S->n) return changed();
        used = at + f.nbytes;
      }
      jobs.push_back({at, at + f.nbytes, f.bs, 0, 1, 0});
      recs.push_back({f.pos, f.bs, 0});
      max_bs = std::max(max_bs, f.bs);
    }
    if (jobs.empty()) return changed();
    if (!ogg) std::memcpy(S->h_buf, S->map + base, (size_t)used);
    for (fl::Job& J : jobs) {
      fl::Header h;
      if (!fl::parse_header(S->h_buf, J.off, J.limit, si.bps, si.max_bs, &h) || h.bs != J.bs) return changed();
      J.hdr = h.len;
    }
    const int m = (int)jobs.size();
    if ((rc = flac_upload(ctx, S, used))) return rc;
    if ((rc = flac_walk<true>(ctx, S, jobs.data(), m, used, res.data()))) return rc;
    for (int j = 0; j < m; j++) {
      if (res[(size_t)j].state != fl::ST_ACCEPT) return changed();
      recs[(size_t)j].ok = 1;
    }
    LDG_TRY(hipMemcpyAsync(S->d_recs, recs.data(), (size_t)m * sizeof(fl::PlaceRec), hipMemcpyHostToDevice, S->st));
    LDG_LAUNCH_ON(S->st, "flac_place", fl::ldg_k_flac_place, dim3((unsigned)((max_bs + 63) / 64), (unsigned)((m + 63) / 64)),
                  256, S->d_scratch, S->nslots, S->d_recs, m, first, n, si.bps, d);
    if ((rc = check_launch(ctx, "ldg_k_flac_place"))) return rc;
    LDG_TRY(hipStreamSynchronize(S->st));
  }
  LDG_TRY(hipStreamSynchronize(S->st));
  prof_collect(ctx);
  return LDG_OK;
}

static int flac_window(ldg_ctx* ctx, const char* fn, ldg_flac_state* S, int64_t first, int64_t n) {
  if (first < 0 || n < 0 || first > S->cnt.nsamples || n > S->cnt.nsamples - first) {
    ctx->err = std::string(fn) + ": the samples asked for are not all within [0, nsamples)";
    return LDG_EINVAL;
  }
  return LDG_OK;
}

int ldg_flac_read(ldg_ctx* ctx, int64_t first_sample, int64_t nsamples, void* dst, int dst_is_device) {
  if (!ctx) return LDG_EINVAL;
  ldg_flac_state* S;
  int rc;
  if ((rc = flac_state(ctx, "ldg_flac_read", true, &S))) return rc;
  if ((rc = flac_window(ctx, "ldg_flac_read", S, first_sample, nsamples))) return rc;
  if (nsamples == 0) return LDG_OK;
  if (!dst) {
    ctx->err = "ldg_flac_read: dst must not be NULL";
    return LDG_EINVAL;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  const int64_t nbytes = nsamples * (S->plan.si.bps / 8);
  if (dst_is_device) return flac_decode_to(ctx, S, first_sample, nsamples, dst);
  if ((rc = flac_buffers(ctx, S, S->buf_bytes))) return rc;
  if (S->tmp_bytes < nbytes) {
    dfree(S->d_tmp);
    S->d_tmp = nullptr;
    S->tmp_bytes = 0;
    if ((rc = dmalloc(ctx, &S->d_tmp, (size_t)nbytes))) return rc;
    S->tmp_bytes = nbytes;
  }
  if ((rc = flac_decode_to(ctx, S, first_sample, nsamples, S->d_tmp))) return rc;
  LDG_TRY(hipMemcpyAsync(dst, S->d_tmp, (size_t)nbytes, hipMemcpyDeviceToHost, S->st));
  LDG_TRY(hipStreamSynchronize(S->st));
  return LDG_OK;
}

int ldg_flac_capture(ldg_ctx* ctx, int64_t first_sample, int64_t nsamples) {
  if (!ctx) return LDG_EINVAL;
  ldg_flac_state* S;
  int rc;
  if ((rc = flac_state(ctx, "ldg_flac_capture", true, &S))) return rc;
  if ((rc = flac_window(ctx, "ldg_flac_capture", S, first_sample, nsamples))) return rc;
  if (nsamples == 0) {
    ctx->err = "ldg_flac_capture: no samples";
    return LDG_EINVAL;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  if ((rc = ldg_stream_close(ctx))) return rc;      // a resident capture replaces a streamed one
  if ((rc = flac_buffers(ctx, S, S->buf_bytes))) return rc;
  const size_t nbytes = (size_t)nsamples * (size_t)(S->plan.si.bps / 8);
  uint8_t* buf = nullptr;
  if ((rc = dmalloc(ctx, &buf, nbytes + 16))) return rc;
  if ((rc = flac_decode_to(ctx, S, first_sample, nsamples, buf))) {
    dfree(buf);
    return rc;
  }
  if (hipError_t e = hipDeviceSynchronize()) {      // no launch still reads the capture this one replaces
    dfree(buf);
    ctx->err = std::string("ldg_flac_capture: hipDeviceSynchronize: ") + hipGetErrorString(e);
    return LDG_EDEVICE;
  }
  if (ctx->cap_owned) dfree(ctx->cap);
  ctx->cap = buf;
  ctx->cap_owned = true;
  ctx->cap_alloc = nbytes;
  ctx->cap_ring = 0;
  ctx->fmt = S->plan.si.bps == 16 ? LDG_FMT_S16 : LDG_FMT_U8;
  ctx->cap_first = first_sample;
  ctx->cap_nsamp = nsamples;
  return LDG_OK;
}

int ldg_flac_close(ldg_ctx* ctx) {
  if (!ctx) return LDG_EINVAL;
  if (ctx->flac) flac_unmap(ctx->flac);
  return LDG_OK;
}
