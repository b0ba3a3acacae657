// Streamed capture (include/ldgpu.h ldg_stream_*): the reference's loader reads each
// 16,384-sample block from the file when the demod needs it (lddutils.py:131-229, called
// per block from RFDecode.demod, lddecode_core.py:373-392), so a capture of any length
// decodes in O(1) memory.  Here a reader thread streams the file, chunk by chunk, through
// pinned staging into a ring in HBM on its own copy stream, ahead of the decode.  What is
// queued, released and waited on is decided by stream_core.hpp (no device call there, so a
// CPU driver tests it); this file holds the device and OS resources and does what the core
// returns.
//
// A chunk may overwrite ring space only once it is released AND the launches that could
// still read it have finished: each release records events on both demod streams, and the
// copy stream waits on the first release record covering the space before the copy.  A
// launch waits (host) until the chunks it reads are queued and (device) on the copy event
// of the last of them, and runs with the window [release, its highest block end): reads
// outside it come back FS_EOF.  No cycle: a launch is issued only after its chunks were
// queued, and every later chunk waits only on launches issued before its release.
#include <fcntl.h>
#include <sys/stat.h>

#include "stream_core.hpp"

struct CapStream {
  int fd = -1;
  uint8_t* ring = nullptr;               // device, R + TAIL bytes
  // Copy streams, chunk c on copy[c % ncopy]: one stream is one DMA engine, and one
  // engine's host-to-device rate is below what the decode consumes (a 60 s u8 step:
  // 1 stream 108 ms, 2 91 ms, 4 86.6 ms against 83 ms resident; profiles/r06_t_*).
  hipStream_t copy[StreamCore::NCOPY_MAX] = {};
  static constexpr int NSTG = 8;
  uint8_t* stg[NSTG] = {};               // pinned staging, chunk bytes each
  hipEvent_t ev_stg[NSTG] = {};
  bool stg_used[NSTG] = {};
  int stg_next = 0;
  std::vector<hipEvent_t> ev_chunk;      // per ring chunk: the copy of its last fill
  hipEvent_t ev_rel[StreamCore::NREL][2] = {};   // release records: events on the two demod streams
  std::thread th;
  static constexpr int NREADERS = 4;     // ReadPool helpers (the box gives a GPU 16 CPUs)
  ReadPool pool;
  StreamCore core;
};

static void stream_reader(ldg_ctx* ctx, CapStream* cs) {
  (void)hipSetDevice(ctx->device);
  StreamCore& core = cs->core;
  StreamCore::Fill f;
  while (core.next_fill(f)) {
    const int k = cs->stg_next;
    cs->stg_next = (k + 1) % CapStream::NSTG;
    const auto ts = std::chrono::steady_clock::now();
    if (cs->stg_used[k] && hipEventSynchronize(cs->ev_stg[k]) != hipSuccess) return core.fail("stream: staging sync");
    const double stage_wait = StreamCore::since(ts);
    const auto t0 = std::chrono::steady_clock::now();
    if (!cs->pool.read(cs->fd, cs->stg[k], f.len, f.fb))
      return core.fail(std::string("stream: read failed in bytes [") + std::to_string(f.fb) + ", " +
                       std::to_string(f.fb + f.len) + ")");
    std::lock_guard<std::mutex> lk(core.mu);
    if (!core.fill_read_locked(f, StreamCore::since(t0), stage_wait)) return;
    hipError_t e = hipSuccess;
    hipStream_t cp = cs->copy[f.copy];
    if (f.rec >= 0) {
      if (e == hipSuccess) e = hipStreamWaitEvent(cp, cs->ev_rel[f.rec][0], 0);
      if (e == hipSuccess) e = hipStreamWaitEvent(cp, cs->ev_rel[f.rec][1], 0);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(cs->ring + f.ro, cs->stg[k], f.len, hipMemcpyHostToDevice, cp);
    if (e == hipSuccess && f.mirror)
      e = hipMemcpyAsync(cs->ring + core.R + f.ro, cs->stg[k], f.mirror, hipMemcpyHostToDevice, cp);
    if (e == hipSuccess) e = hipEventRecord(cs->ev_stg[k], cp);
    if (e == hipSuccess) e = hipEventRecord(cs->ev_chunk[f.slot], cp);
    if (e != hipSuccess) return core.fail_locked(std::string("stream: ") + hipGetErrorString(e));
    cs->stg_used[k] = true;
    core.fill_queued_locked(f);
  }
}

static void stream_stop(CapStream* cs) {
  cs->core.request_stop();
  if (cs->th.joinable()) cs->th.join();
}

// The one place that points the context's capture at the ring (window [first, first + nsamp))
static void stream_attach(ldg_ctx* ctx, const CapStream* cs, int64_t first, int64_t nsamp) {
  ctx->cap = cs->ring;
  ctx->cap_ring = cs->core.R;
  ctx->cap_first = first;
  ctx->cap_nsamp = nsamp;
}

// ... and away from it
static void stream_detach(ldg_ctx* ctx, const CapStream* cs) {
  if (ctx->cap != cs->ring) return;
  ctx->cap = nullptr;
  ctx->cap_ring = 0;
}

static void stream_free(ldg_ctx* ctx, CapStream* cs) {
  if (!cs) return;
  stream_stop(cs);
  cs->pool.stop();
  (void)hipSetDevice(ctx->device);
  for (hipStream_t c : cs->copy)
    if (c) (void)hipStreamSynchronize(c);
  for (hipStream_t st : {ctx->stream, ctx->stream_b})
    if (st) (void)hipStreamSynchronize(st);
  for (auto e : cs->ev_chunk)
    if (e) (void)hipEventDestroy(e);
  for (auto& pr : cs->ev_rel)
    for (auto e : pr)
      if (e) (void)hipEventDestroy(e);
  for (int k = 0; k < CapStream::NSTG; k++) {
    if (cs->ev_stg[k]) (void)hipEventDestroy(cs->ev_stg[k]);
    if (cs->stg[k]) (void)hipHostFree(cs->stg[k]);
  }
  for (hipStream_t c : cs->copy)
    if (c) (void)hipStreamDestroy(c);
  if (cs->ring) (void)hipFree(cs->ring);
  if (cs->fd >= 0) close(cs->fd);
  stream_detach(ctx, cs);
  delete cs;
}

// (Re)start the reader at the packing group holding `sample`: nothing of the old window
// is kept.  The caller has no decode outstanding that reads the ring.
static int stream_restart(ldg_ctx* ctx, CapStream* cs, int64_t sample) {
  stream_stop(cs);
  for (int j = 0; j < cs->core.ncopy; j++) LDG_TRY(hipStreamSynchronize(cs->copy[j]));
  LDG_TRY(hipStreamSynchronize(ctx->stream));
  LDG_TRY(hipStreamSynchronize(ctx->stream_b));
  cs->core.restart(sample);
  cs->th = std::thread(stream_reader, ctx, cs);
  return LDG_OK;
}

// Before a launch on stream s whose blocks read samples up to hi: wait until the reader has
// queued them, make s wait for their copy, and set the kernels' capture window (its low end
// is the released point).
static int stream_prepare(ldg_ctx* ctx, hipStream_t s, int64_t hi) {
  CapStream* cs = ctx->cs;
  StreamCore::Launch l;
  {
    std::unique_lock<std::mutex> lk(cs->core.mu);
    l = cs->core.prepare_locked(lk, hi, std::chrono::seconds(60));
    if (l.st != StreamCore::OK) {
      ctx->err = l.err;
      return l.st == StreamCore::PAST_RING ? LDG_ESTATE : LDG_EDEVICE;
    }
    for (int i = 0; i < l.nslot; i++) LDG_TRY(hipStreamWaitEvent(s, cs->ev_chunk[l.slot[i]], 0));
  }
  stream_attach(ctx, cs, l.win_lo, l.win_hi - l.win_lo);
  return LDG_OK;
}

extern "C" {

int ldg_stream_open(ldg_ctx* ctx, const char* path, int fmt, int64_t ring_bytes, int64_t first_sample) {
  if (!ctx || !path || fmt < 0 || fmt > 3 || ring_bytes <= 0 || first_sample < 0) return LDG_EINVAL;
  if (ctx->ncalls) {
    ctx->err = "stream: open with decodes outstanding";
    return LDG_ESTATE;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  const int fd = open(path, O_RDONLY);
  struct stat st {};
  if (fd < 0 || fstat(fd, &st) != 0) {
    if (fd >= 0) close(fd);
    ctx->err = std::string("stream: cannot open ") + path;
    return LDG_EINVAL;
  }
  int ncopy = StreamCore::NCOPY_MAX;
  if (const char* nc = getenv("LDG_STREAM_COPIES"))   // tuning: copy streams (1 - 4)
    ncopy = std::max(1, std::min(StreamCore::NCOPY_MAX, atoi(nc)));
  CapStream* cs = ctx->cs;
  int rc = LDG_OK;
  if (cs && cs->core.same_ring(ring_bytes, ncopy)) {
    // the same ring again (the next file of a job): keep its memory, streams and events
    stream_stop(cs);
    close(cs->fd);
  } else {
    stream_free(ctx, cs);
    ctx->cs = nullptr;
    cs = new CapStream();
    cs->pool.start(CapStream::NREADERS);
    if (!cs->core.configure(ring_bytes, ncopy)) {
      close(fd);
      ctx->err = "stream: ring too small (at least 4 x 64 KiB)";
      stream_free(ctx, cs);
      return LDG_EINVAL;
    }
    const StreamCore& core = cs->core;
    if (hipMalloc(&cs->ring, (size_t)(core.R + StreamCore::TAIL)) != hipSuccess) rc = LDG_ENOMEM;
    for (int j = 0; j < core.ncopy && !rc; j++)
      if (hipStreamCreateWithFlags(&cs->copy[j], hipStreamNonBlocking) != hipSuccess) rc = LDG_EDEVICE;
    for (int k = 0; k < CapStream::NSTG && !rc; k++)
      if (hipHostMalloc((void**)&cs->stg[k], (size_t)core.chunk, hipHostMallocDefault) != hipSuccess ||
          hipEventCreateWithFlags(&cs->ev_stg[k], hipEventDisableTiming) != hipSuccess)
        rc = LDG_ENOMEM;
    cs->ev_chunk.assign((size_t)(core.R / core.chunk), nullptr);
    for (auto& e : cs->ev_chunk)
      if (!rc && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) rc = LDG_EDEVICE;
    for (int i = 0; i < StreamCore::NREL && !rc; i++)
      for (auto& e : cs->ev_rel[i])
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) rc = LDG_EDEVICE;
    if (!rc && ctx->cap_owned) {                      // the streamed capture replaces a resident one
      dfree(ctx->cap);
      ctx->cap = nullptr;
      ctx->cap_alloc = 0;
      ctx->cap_owned = false;
    }
  }
  cs->fd = fd;
  cs->core.set_file(st.st_size, fmt);
  if (!rc) {
    ctx->cs = cs;
    ctx->fmt = fmt;
    rc = stream_restart(ctx, cs, first_sample);
  }
  if (!rc) {
    stream_attach(ctx, cs, cs->core.sample_ceil(cs->core.base_b), 0);
    return LDG_OK;
  }
  // no stream without a reader is left behind: the next launch would wait for it
  if (rc == LDG_ENOMEM) ctx->err = "stream: out of memory for the ring or its staging";
  stream_free(ctx, cs);
  ctx->cs = nullptr;
  return rc;
}

int ldg_stream_release(ldg_ctx* ctx, int64_t below_sample) {
  if (!ctx || !ctx->cs) return LDG_ESTATE;
  CapStream* cs = ctx->cs;
  const int64_t b = cs->core.release_byte(below_sample);
  std::lock_guard<std::mutex> lk(cs->core.mu);
  const int idx = cs->core.release_pick_locked(b);
  if (idx < 0) return LDG_OK;
  LDG_TRY(hipEventRecord(cs->ev_rel[idx][0], ctx->stream));
  LDG_TRY(hipEventRecord(cs->ev_rel[idx][1], ctx->stream_b));
  cs->core.release_commit_locked(b);
  return LDG_OK;
}

int ldg_stream_seek(ldg_ctx* ctx, int64_t first_sample) {
  if (!ctx || !ctx->cs || first_sample < 0) return LDG_EINVAL;
  if (ctx->ncalls) {
    ctx->err = "stream: seek with decodes outstanding";
    return LDG_ESTATE;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  ctx->cs->core.seeks++;
  return stream_restart(ctx, ctx->cs, first_sample);
}

int ldg_stream_window(ldg_ctx* ctx, int64_t* out4) {
  if (!ctx || !ctx->cs || !out4) return LDG_ESTATE;
  ctx->cs->core.window(out4);
  return LDG_OK;
}

int ldg_stream_stats(ldg_ctx* ctx, double* out, int n) {
  if (!ctx || !ctx->cs || !out || n <= 0) return LDG_ESTATE;
  return ctx->cs->core.stats(out, n);
}

int ldg_stream_close(ldg_ctx* ctx) {
  if (!ctx) return LDG_EINVAL;
  if (!ctx->cs) return LDG_OK;
  (void)hipSetDevice(ctx->device);
  stream_free(ctx, ctx->cs);
  ctx->cs = nullptr;
  return LDG_OK;
}

}  // extern "C"
