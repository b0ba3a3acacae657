// Host side of the EFM run-length extraction (efm.hip; build-defined, DESIGN.md section 7c):
// ldg_efm_* of include/ldgpu.h.  Unity-built after abi.inc.

struct ldg_efm_state {
  ldg_efm_opts opts;
  bool have_taps = false;
  hipStream_t st = nullptr;
  double* d_taps = nullptr;
  // grown on demand, never shrunk
  uint8_t* d_raw = nullptr;      size_t raw_cap = 0;     // a host window's bytes
  double* d_y = nullptr;         size_t y_cap = 0;       // FIR tiles' outputs
  double* d_B = nullptr;         size_t b_cap = 0;       // their block sums
  int32_t* d_cnt = nullptr;      size_t ct_cap = 0;      // crossing tiles' counts
  int64_t* d_off = nullptr;                              // and offsets (ct_cap), then the two totals
  double* d_t = nullptr;         size_t t_cap = 0;       // crossing times (one per z at the most)
  uint8_t* d_tmp = nullptr;                              // per-segment bytes (t_cap)
  uint8_t* d_out = nullptr;                              // packed bytes (t_cap)
  double* d_z = nullptr;         size_t z_cap = 0;       // z (opts.keep_debug only)
  ldg::efm::SegDev* d_segs = nullptr; size_t seg_cap = 0;
  // the last call, for ldg_efm_debug_read
  int64_t last_z_lo = 0, last_nz = 0, last_ncross = 0;
  bool last_has_z = false;
};

namespace {

template <class T>
int efm_grow(ldg_ctx* ctx, T** p, size_t* cap, size_t need) {
  if (need <= *cap) return LDG_OK;
  dfree(*p);
  *p = nullptr;
  *cap = 0;
  if (int rc = dmalloc(ctx, p, need)) return rc;
  *cap = need;
  return LDG_OK;
}

int64_t efm_sample_byte(int fmt, int64_t s) {   // byte offset of sample s (s on a group boundary)
  return fmt == LDG_FMT_U8 ? s : fmt == LDG_FMT_S16 ? 2 * s : fmt == LDG_FMT_R30 ? s / 3 * 4 : s / 4 * 5;
}

int64_t efm_samples_in(int fmt, int64_t nbytes) {
  return fmt == LDG_FMT_U8 ? nbytes : fmt == LDG_FMT_S16 ? nbytes / 2 : fmt == LDG_FMT_R30 ? nbytes / 4 * 3 : nbytes / 5 * 4;
}

}  // namespace

static void efm_free(ldg_ctx* ctx) {
  ldg_efm_state* E = ctx->efm;
  if (!E) return;
  if (E->st) {
    (void)hipStreamSynchronize(E->st);
    (void)hipStreamDestroy(E->st);
  }
  for (void* p : {(void*)E->d_taps, (void*)E->d_raw, (void*)E->d_y, (void*)E->d_B, (void*)E->d_cnt, (void*)E->d_off,
                  (void*)E->d_t, (void*)E->d_tmp, (void*)E->d_out, (void*)E->d_z, (void*)E->d_segs})
    dfree(p);
  delete E;
  ctx->efm = nullptr;
}

extern "C" {

int ldg_efm_defaults(ldg_efm_opts* out) {
  if (!out) return LDG_EINVAL;
  out->fs = 40e6;
  out->alpha = 0.1;      // the sweep of DESIGN.md section 7c (tests/efm_ref.py sweep())
  out->beta = 0.002;
  out->delta = 0.03;
  out->keep_debug = 0;
  out->pad_ = 0;
  return LDG_OK;
}

int ldg_efm_window(int64_t seg_lo, int64_t seg_hi, int64_t file_nsamples, int64_t out[2]) {
  if (!out) return LDG_EINVAL;
  ldg::efm::Plan p;
  if (ldg::efm::plan(seg_lo, seg_hi, file_nsamples, &p)) return LDG_EINVAL;
  out[0] = p.win_lo;
  out[1] = p.win_hi;
  return LDG_OK;
}

int ldg_efm_set_opts(ldg_ctx* ctx, const ldg_efm_opts* opts, const double* taps, int ntaps) {
  if (!ctx) return LDG_EINVAL;
  auto bad = [&](const char* what) {
    ctx->err = std::string("ldg_efm_set_opts: ") + what;
    return LDG_EINVAL;
  };
  if (!opts || !taps) return bad("opts and taps are required");
  if (ntaps != ldg::efm::NTAPS) return bad("ntaps must be 255");
  if (!(opts->fs > 0) || !(opts->alpha >= 0 && opts->alpha <= 1) || !(opts->beta >= 0 && opts->beta <= 1) ||
      !(opts->delta >= 0 && opts->delta < 1))
    return bad("fs > 0, alpha and beta in [0, 1], delta in [0, 1)");
  for (int k = 0; k < ntaps; k++)
    if (!std::isfinite(taps[k])) return bad("a tap is not finite");
  LDG_TRY(hipSetDevice(ctx->device));
  if (!ctx->efm) ctx->efm = new ldg_efm_state();
  ldg_efm_state* E = ctx->efm;
  if (!E->st && hipStreamCreateWithFlags(&E->st, hipStreamNonBlocking) != hipSuccess) {
    E->st = nullptr;
    ctx->err = "EFM: hipStreamCreate failed";
    return LDG_EDEVICE;
  }
  LDG_TRY(hipStreamSynchronize(E->st));
  if (int rc = upload_f64(ctx, &E->d_taps, taps, (size_t)ntaps)) return rc;
  E->opts = *opts;
  E->have_taps = true;
  return LDG_OK;
}

int ldg_efm_extract(ldg_ctx* ctx, const void* raw, int64_t nbytes, int fmt, int64_t first_sample, int64_t file_nsamples,
                    int64_t seg_lo, int64_t seg_hi, uint8_t* out, int64_t cap, int64_t* n_out, ldg_efm_seg* per_segment) {
  using namespace ldg::efm;
  if (!ctx) return LDG_EINVAL;
  auto bad = [&](const char* what) {
    ctx->err = std::string("ldg_efm_extract: ") + what;
    return LDG_EINVAL;
  };
  ldg_efm_state* E = ctx->efm;
  if (!E || !E->have_taps) {
    ctx->err = "ldg_efm_extract: ldg_efm_set_opts has not been called";
    return LDG_ESTATE;
  }
  if (!n_out || !per_segment || cap < 0 || (cap > 0 && !out)) return bad("out, n_out and per_segment are required");
  if (fmt < LDG_FMT_U8 || fmt > LDG_FMT_LDS) return bad("unknown format");
  if (nbytes < 0 || first_sample < 0 || (nbytes > 0 && !raw)) return bad("the window is invalid");
  if ((fmt == LDG_FMT_R30 && first_sample % 3) || (fmt == LDG_FMT_LDS && first_sample % 4))
    return bad("first_sample must lie on a packing group (3 samples .r30, 4 samples .lds)");
  Plan P;
  if (plan(seg_lo, seg_hi, file_nsamples, &P)) return bad("the segment range is invalid");
  const int64_t nseg = seg_hi - seg_lo;
  if (nseg > 65535) return bad("at most 65535 segments a call");
  const int64_t win_n = efm_samples_in(fmt, nbytes);
  if (P.need_hi > P.need_lo && (first_sample > P.need_lo || first_sample + win_n < P.need_hi)) {
    ctx->err = "ldg_efm_extract: the window [" + std::to_string(first_sample) + ", " + std::to_string(first_sample + win_n) +
               ") does not cover the samples the segments need [" + std::to_string(P.need_lo) + ", " +
               std::to_string(P.need_hi) + ") (ldg_efm_window)";
    return LDG_EINVAL;
  }
  *n_out = 0;
  E->last_nz = E->last_ncross = 0;
  E->last_has_z = false;
  const double p0 = E->opts.fs / CHANNEL_HZ;
  if (nseg == 0) return LDG_OK;
  if (P.z_hi < P.z_lo) {     // the file defines no z here: every segment is empty
    for (int64_t i = 0; i < nseg; i++) per_segment[i] = ldg_efm_seg{0, 0, 0, 0, p0};
    return LDG_OK;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  hipStream_t st = E->st;
  // the window on the device
  const uint8_t* d_raw = nullptr;
  {
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, raw);
    bool on_device = false;
    if (e == hipSuccess) on_device = at.type == hipMemoryTypeDevice;
    else (void)hipGetLastError();      // plain host memory is no error
    if (on_device) {
      d_raw = static_cast<const uint8_t*>(raw);
    } else {
      if (int rc = efm_grow(ctx, &E->d_raw, &E->raw_cap, (size_t)nbytes)) return rc;
      LDG_TRY(hipMemcpyAsync(E->d_raw, raw, (size_t)nbytes, hipMemcpyHostToDevice, st));
      d_raw = E->d_raw;
    }
  }
  const int64_t ntile = P.tile_hi - P.tile_lo, nct = P.ctile_hi - P.ctile_lo, nz = P.z_hi - P.z_lo + 1;
  if (int rc = efm_grow(ctx, &E->d_y, &E->y_cap, (size_t)ntile * TILE)) return rc;
  if (int rc = efm_grow(ctx, &E->d_B, &E->b_cap, (size_t)ntile * BLOCKS_PER_TILE)) return rc;
  if ((size_t)nct > E->ct_cap) {
    dfree(E->d_off);
    E->d_off = nullptr;
    if (int rc = efm_grow(ctx, &E->d_cnt, &E->ct_cap, (size_t)nct)) return rc;
    if (int rc = dmalloc(ctx, &E->d_off, (size_t)nct + 2)) {
      E->ct_cap = 0;
      return rc;
    }
  }
  if ((size_t)nz > E->t_cap) {
    dfree(E->d_tmp);
    dfree(E->d_out);
    E->d_tmp = E->d_out = nullptr;
    if (int rc = efm_grow(ctx, &E->d_t, &E->t_cap, (size_t)nz)) return rc;
    if (dmalloc(ctx, &E->d_tmp, (size_t)nz) || dmalloc(ctx, &E->d_out, (size_t)nz)) {
      E->t_cap = 0;
      return LDG_ENOMEM;
    }
  }
  const bool keep = E->opts.keep_debug != 0;
  if (keep)
    if (int rc = efm_grow(ctx, &E->d_z, &E->z_cap, (size_t)nz)) return rc;
  if (int rc = efm_grow(ctx, &E->d_segs, &E->seg_cap, (size_t)nseg)) return rc;
  int64_t* d_ncross = E->d_off + E->ct_cap;
  int64_t* d_nbytes = d_ncross + 1;
  const int64_t y_off = P.tile_lo * TILE, b_off = P.tile_lo * BLOCKS_PER_TILE;

  LDG_LAUNCH_ON(st, "efm_fir", ldg_k_efm_fir, dim3((unsigned)ntile), FIR_THREADS, d_raw, fmt, first_sample, win_n,
                E->d_taps, P.tile_lo, E->d_y, y_off, E->d_B, b_off);
  LDG_LAUNCH_ON(st, "efm_cross_count", ldg_k_efm_cross<false>, dim3((unsigned)nct), 256, E->d_y, y_off, E->d_B, b_off,
                P.z_lo, P.z_hi, P.ctile_lo, E->d_cnt, (const int64_t*)nullptr, (double*)nullptr, (double*)nullptr);
  LDG_LAUNCH_ON(st, "efm_scan", ldg_k_efm_scan, dim3(1), 1024, E->d_cnt, nct, E->d_off, d_ncross);
  LDG_LAUNCH_ON(st, "efm_cross_write", ldg_k_efm_cross<true>, dim3((unsigned)nct), 256, E->d_y, y_off, E->d_B, b_off,
                P.z_lo, P.z_hi, P.ctile_lo, (int32_t*)nullptr, E->d_off, E->d_t, keep ? E->d_z : (double*)nullptr);
  ClockArgs A{p0, p0 * (1.0 - E->opts.delta), p0 * (1.0 + E->opts.delta), E->opts.alpha, E->opts.beta};
  LDG_LAUNCH_ON(st, "efm_clock", ldg_k_efm_clock, dim3((unsigned)nseg), 64, E->d_t, d_ncross, seg_lo, A, E->d_tmp,
                E->d_segs);
  LDG_LAUNCH_ON(st, "efm_offsets", ldg_k_efm_offsets, dim3(1), 64, E->d_segs, nseg, d_nbytes);
  LDG_LAUNCH_ON(st, "efm_pack", ldg_k_efm_pack, dim3((unsigned)nseg, 8), 256, E->d_segs, E->d_tmp, E->d_out, (int64_t)E->t_cap);
  if (int rc = check_launch(ctx, "ldg_k_efm_*")) return rc;
  int64_t tot[2] = {0, 0};
  std::vector<SegDev> segs((size_t)nseg);
  LDG_TRY(hipMemcpyAsync(tot, d_ncross, sizeof(tot), hipMemcpyDeviceToHost, st));
  LDG_TRY(hipMemcpyAsync(segs.data(), E->d_segs, (size_t)nseg * sizeof(SegDev), hipMemcpyDeviceToHost, st));
  LDG_TRY(hipStreamSynchronize(st));
  prof_collect(ctx);
  E->last_z_lo = P.z_lo;
  E->last_nz = nz;
  E->last_ncross = tot[0];
  E->last_has_z = keep;
  for (int64_t i = 0; i < nseg; i++)
    per_segment[i] = ldg_efm_seg{segs[i].emitted, segs[i].ignored, segs[i].clamped_low, segs[i].clamped_high, segs[i].final_P};
  *n_out = tot[1];
  if (tot[1] > cap) {
    ctx->err = "ldg_efm_extract: the output needs " + std::to_string(tot[1]) + " bytes, out holds " + std::to_string(cap);
    return LDG_EINVAL;
  }
  if (tot[1] > 0) LDG_TRY(hipMemcpy(out, E->d_out, (size_t)tot[1], hipMemcpyDeviceToHost));
  return LDG_OK;
}

int64_t ldg_efm_debug_read(ldg_ctx* ctx, int what, void* dst, int64_t cap, int64_t* first) {
  if (!ctx || !dst || cap < 0 || !ctx->efm) return LDG_EINVAL;
  ldg_efm_state* E = ctx->efm;
  const void* src;
  int64_t bytes;
  if (what == 0) {
    if (!E->last_has_z) return LDG_ESTATE;
    src = E->d_z;
    bytes = E->last_nz * 8;
    if (first) *first = E->last_z_lo;
  } else if (what == 1) {
    src = E->d_t;
    bytes = E->last_ncross * 8;
    if (first) *first = 0;
  } else {
    return LDG_EINVAL;
  }
  if (bytes > cap) bytes = cap;
  if (bytes == 0) return 0;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(E->st) != hipSuccess) return LDG_EDEVICE;
  if (hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) return LDG_EDEVICE;
  return bytes;
}

}  // extern "C"
