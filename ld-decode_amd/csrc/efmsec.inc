// Host side of the EFM data sectors (efmsec.hip; build-defined, DESIGN.md section 7e):
// ldg_efmsec_* of include/ldgpu.h.  Unity-built after efmdec.inc (efm_grow is efm.inc's), which
// hands the stage each call's frames through efmsec_take.

struct ldg_efmsec_state {
  bool enabled = false;                                   // ldg_efmdec_feed feeds the stage
  bool ready = false;                                     // the tables are on the device
  hipStream_t st = nullptr;
  uint8_t* d_gf = nullptr;
  uint8_t* d_scr = nullptr;                               // the scrambler's 2340 bytes
  uint32_t* d_xp = nullptr;                               // the EDC lanes' powers of x
  unsigned long long* d_counters = nullptr;
  ldg::efmsec::GridOut* d_grid = nullptr;
  int64_t* d_tot = nullptr;                               // a scan's total
  // the stream between calls (efmsec_plan.hpp): the bytes held are d_by[cur] + off .. + held
  ldg::efmsec::Carry carry;
  int cur = 0;
  int64_t off = 0, held = 0, nsec = 0;
  bool ended = false;
  // grown on demand, never shrunk
  uint8_t* d_by[2] = {nullptr, nullptr};   size_t by_cap[2] = {0, 0};
  uint8_t* d_er[2] = {nullptr, nullptr};   size_t er_cap[2] = {0, 0};
  int64_t* d_cand = nullptr;     size_t cand_cap = 0;
  int64_t* d_conf = nullptr;     size_t conf_cap = 0;
  int64_t* d_starts = nullptr;   size_t starts_cap = 0;
  int32_t* d_cnt[2] = {nullptr, nullptr};  size_t cnt_cap[2] = {0, 0};   // tiles' counts
  int64_t* d_off[2] = {nullptr, nullptr};  size_t off_cap[2] = {0, 0};   // and offsets
  uint8_t* d_sectors = nullptr;  size_t sectors_cap = 0;
  uint8_t* d_data = nullptr;     size_t data_cap = 0;
  ldg::efmsec::Rec* d_recs = nullptr;      size_t recs_cap = 0;
  // the last call, for ldg_efmsec_read and ldg_efmsec_last_info
  int64_t last_new_at = 0, last_new = 0, last_sectors = 0;
  ldg_efmsec_info last{};
};

static_assert(sizeof(ldg::efmsec::Rec) == sizeof(ldg_efmsec_rec), "ldg_efmsec_rec is the kernel's record");

static void efmsec_free(ldg_ctx* ctx) {
  ldg_efmsec_state* S = ctx->efmsec;
  if (!S) return;
  if (S->st) {
    (void)hipStreamSynchronize(S->st);
    (void)hipStreamDestroy(S->st);
  }
  for (void* p : {(void*)S->d_gf, (void*)S->d_scr, (void*)S->d_xp, (void*)S->d_counters, (void*)S->d_grid, (void*)S->d_tot,
                  (void*)S->d_by[0], (void*)S->d_by[1], (void*)S->d_er[0], (void*)S->d_er[1], (void*)S->d_cand,
                  (void*)S->d_conf, (void*)S->d_starts, (void*)S->d_cnt[0], (void*)S->d_cnt[1], (void*)S->d_off[0],
                  (void*)S->d_off[1], (void*)S->d_sectors, (void*)S->d_data, (void*)S->d_recs})
    dfree(p);
  delete S;
  ctx->efmsec = nullptr;
}

static bool efmsec_enabled(ldg_ctx* ctx) { return ctx->efmsec && ctx->efmsec->enabled; }

static void efmsec_restart(ldg_ctx* ctx) {
  ldg_efmsec_state* S = ctx->efmsec;
  if (!S) return;
  S->carry = ldg::efmsec::Carry();
  S->off = S->held = S->nsec = 0;
  S->ended = false;
  S->last_new_at = S->last_new = S->last_sectors = 0;
  S->last = ldg_efmsec_info{};
}

namespace {

// the state, allocated on first use: the stream and the three tables
int efmsec_state(ldg_ctx* ctx, ldg_efmsec_state** out) {
  using namespace ldg::efmsec;
  LDG_TRY(hipSetDevice(ctx->device));
  if (!ctx->efmsec) ctx->efmsec = new ldg_efmsec_state();
  ldg_efmsec_state* S = ctx->efmsec;
  *out = S;
  if (S->ready) return LDG_OK;
  if (!S->st && hipStreamCreateWithFlags(&S->st, hipStreamNonBlocking) != hipSuccess) {
    S->st = nullptr;
    ctx->err = "EFM sectors: hipStreamCreate failed";
    return LDG_EDEVICE;
  }
  // (a call that failed half way left some of these allocated)
  if (!S->d_gf) if (int rc = dmalloc(ctx, &S->d_gf, (size_t)GF_BYTES)) return rc;
  if (!S->d_scr) if (int rc = dmalloc(ctx, &S->d_scr, (size_t)(SECTOR - 12))) return rc;
  if (!S->d_xp) if (int rc = dmalloc(ctx, &S->d_xp, (size_t)EDC_LANES)) return rc;
  if (!S->d_counters) if (int rc = dmalloc(ctx, &S->d_counters, (size_t)K_COUNT)) return rc;
  if (!S->d_grid) if (int rc = dmalloc(ctx, &S->d_grid, 1)) return rc;
  if (!S->d_tot) if (int rc = dmalloc(ctx, &S->d_tot, 1)) return rc;
  uint8_t gf[GF_BYTES] = {0};       // antilog, doubled, then log: polynomial 0x11d, alpha = 2 (as efmdec.inc)
  unsigned x = 1;
  for (int i = 0; i < 255; i++) {
    gf[i] = gf[i + 255] = (uint8_t)x;
    gf[512 + x] = (uint8_t)i;
    x <<= 1;
    if (x & 0x100) x ^= 0x11d;
  }
  gf[510] = gf[0];
  gf[511] = gf[1];
  uint8_t scr[SECTOR - 12];         // x^15 + x + 1, preset 0x0001, LSB first
  unsigned reg = 1;
  for (int i = 0; i < (int)(SECTOR - 12); i++) {
    unsigned b = 0;
    for (int k = 0; k < 8; k++) {
      b |= (reg & 1u) << k;
      reg = (reg >> 1) | (((reg ^ (reg >> 1)) & 1u) << 14);
    }
    scr[i] = (uint8_t)b;
  }
  uint32_t xp[EDC_LANES];           // lane i: x^(8 * bytes after its twelve), reflected (bit 31 is x^0)
  uint32_t p = 0x80000000u;
  for (int i = EDC_LANES - 1; i >= 0; i--) {
    xp[i] = p;
    for (int k = 0; k < 8 * EDC_CHUNK; k++) p = (p >> 1) ^ ((p & 1u) ? EDC_POLY : 0u);
  }
  LDG_TRY(hipMemcpy(S->d_gf, gf, sizeof(gf), hipMemcpyHostToDevice));
  LDG_TRY(hipMemcpy(S->d_scr, scr, sizeof(scr), hipMemcpyHostToDevice));
  LDG_TRY(hipMemcpy(S->d_xp, xp, sizeof(xp), hipMemcpyHostToDevice));
  S->ready = true;
  return LDG_OK;
}

int efmsec_total(ldg_ctx* ctx, ldg_efmsec_state* S, int64_t* out) {
  LDG_TRY(hipMemcpyAsync(out, S->d_tot, sizeof(int64_t), hipMemcpyDeviceToHost, S->st));
  LDG_TRY(hipStreamSynchronize(S->st));
  return LDG_OK;
}

// One call: n new bytes, from host arrays (hby, her) or gathered from C2 rows on the device
// (c2, c2f: local frame `first` on; the caller's stream has finished with them).
int efmsec_run(ldg_ctx* ctx, ldg_efmsec_state* S, const uint8_t* hby, const uint8_t* her, const uint8_t* c2,
               const uint32_t* c2f, int64_t first, int64_t n, bool fin, ldg_efmsec_info* info) {
  using namespace ldg::efmsec;
  if (S->ended) {
    ctx->err = "ldg_efmsec_feed: the stream has ended (ldg_efmsec_reset starts another)";
    return LDG_ESTATE;
  }
  if (S->held + n > ((int64_t)1 << 31) - 4096) {
    ctx->err = "ldg_efmsec_feed: at most 2^31 bytes held in a call";
    return LDG_EINVAL;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  hipStream_t st = S->st;
  const int nxt = S->cur ^ 1;
  const int64_t held = S->held, nb = held + n, pos0 = S->carry.pos0;
  if (int rc = efm_grow(ctx, &S->d_by[nxt], &S->by_cap[nxt], (size_t)nb + 1)) return rc;
  if (int rc = efm_grow(ctx, &S->d_er[nxt], &S->er_cap[nxt], (size_t)nb + 1)) return rc;
  uint8_t* by = S->d_by[nxt];
  uint8_t* er = S->d_er[nxt];
  if (held > 0) {
    LDG_TRY(hipMemcpyAsync(by, S->d_by[S->cur] + S->off, (size_t)held, hipMemcpyDeviceToDevice, st));
    LDG_TRY(hipMemcpyAsync(er, S->d_er[S->cur] + S->off, (size_t)held, hipMemcpyDeviceToDevice, st));
  }
  if (n > 0 && hby) {
    LDG_TRY(hipMemcpyAsync(by + held, hby, (size_t)n, hipMemcpyHostToDevice, st));
    LDG_TRY(hipMemcpyAsync(er + held, her, (size_t)n, hipMemcpyHostToDevice, st));
  } else if (n > 0) {
    LDG_LAUNCH_ON(st, "efmsec_gather", ldg_k_efmsec_gather, dim3((unsigned)((n + 255) / 256)), 256, c2, c2f, first, n,
                  by + held, er + held);
  }
  LDG_TRY(hipMemsetAsync(S->d_counters, 0, K_COUNT * sizeof(unsigned long long), st));

  // ---- the sector grid over the held bytes and the new ones ----
  const Window w = window_of(S->carry, pos0 + nb, fin);
  int64_t ncand = 0, nconf = 0, ns = 0;
  GridOut g{fin ? NEVER : S->carry.emit_from, pos0, 0, 0, 0};
  if (nb > 0) {
    const int64_t ct = (nb + CAND_TILE - 1) / CAND_TILE;
    // the pairs also hold the candidates' and the confirmed candidates' tiles of 256 (a candidate takes 11 bytes)
    for (int q = 0; q < 2; q++) {
      if (int rc = efm_grow(ctx, &S->d_cnt[q], &S->cnt_cap[q], (size_t)(nb / 256 + 1))) return rc;
      if (int rc = efm_grow(ctx, &S->d_off[q], &S->off_cap[q], (size_t)(nb / 256 + 1))) return rc;
    }
    LDG_LAUNCH_ON(st, "efmsec_cand_count", ldg_k_efmsec_cand<false>, dim3((unsigned)ct), 256, by, nb, pos0, S->d_cnt[0],
                  (const int64_t*)nullptr, (int64_t*)nullptr);
    LDG_LAUNCH_ON(st, "efmsec_scan", ldg::efm::ldg_k_efm_scan, dim3(1), 1024, S->d_cnt[0], ct, S->d_off[0], S->d_tot);
    if (int rc = check_launch(ctx, "ldg_k_efmsec_cand")) return rc;
    if (int rc = efmsec_total(ctx, S, &ncand)) return rc;
    if (int rc = efm_grow(ctx, &S->d_cand, &S->cand_cap, (size_t)ncand + 1)) return rc;
    if (int rc = efm_grow(ctx, &S->d_conf, &S->conf_cap, (size_t)ncand + 1)) return rc;
    if (ncand > 0) {
      LDG_LAUNCH_ON(st, "efmsec_cand_write", ldg_k_efmsec_cand<true>, dim3((unsigned)ct), 256, by, nb, pos0, (int32_t*)nullptr,
                    S->d_off[0], S->d_cand);
      const int64_t kt = (ncand + 255) / 256;
      LDG_LAUNCH_ON(st, "efmsec_confirm_count", ldg_k_efmsec_confirm<false>, dim3((unsigned)kt), 256, S->d_cand, ncand,
                    S->d_cnt[1], (const int64_t*)nullptr, (int64_t*)nullptr);
      LDG_LAUNCH_ON(st, "efmsec_scan", ldg::efm::ldg_k_efm_scan, dim3(1), 1024, S->d_cnt[1], kt, S->d_off[1], S->d_tot);
      LDG_LAUNCH_ON(st, "efmsec_confirm_write", ldg_k_efmsec_confirm<true>, dim3((unsigned)kt), 256, S->d_cand, ncand,
                    (int32_t*)nullptr, S->d_off[1], S->d_conf);
      if (int rc = check_launch(ctx, "ldg_k_efmsec_confirm")) return rc;
      if (int rc = efmsec_total(ctx, S, &nconf)) return rc;
    }
    const int64_t ft = (nconf + 255) / 256;
    if (nconf > 0) {
      LDG_LAUNCH_ON(st, "efmsec_sectors_count", ldg_k_efmsec_sectors<false>, dim3((unsigned)ft), 256, S->d_conf, nconf, w,
                    S->d_cnt[0], (const int64_t*)nullptr, (int64_t*)nullptr, S->d_counters);
      LDG_LAUNCH_ON(st, "efmsec_scan", ldg::efm::ldg_k_efm_scan, dim3(1), 1024, S->d_cnt[0], ft, S->d_off[0], S->d_tot);
    }
    LDG_LAUNCH_ON(st, "efmsec_finish", ldg_k_efmsec_finish, dim3(1), 64, pos0, S->d_cand, ncand, S->d_conf, nconf, w,
                  S->d_grid);
    if (int rc = check_launch(ctx, "ldg_k_efmsec_sectors")) return rc;
    LDG_TRY(hipMemcpyAsync(&g, S->d_grid, sizeof(g), hipMemcpyDeviceToHost, st));
    if (nconf > 0) {
      if (int rc = efmsec_total(ctx, S, &ns)) return rc;
    } else {
      LDG_TRY(hipStreamSynchronize(st));
    }
    // ---- the sectors ----
    if (ns > 0) {
      if (int rc = efm_grow(ctx, &S->d_starts, &S->starts_cap, (size_t)ns)) return rc;
      if (int rc = efm_grow(ctx, &S->d_sectors, &S->sectors_cap, (size_t)ns * SECTOR)) return rc;
      if (int rc = efm_grow(ctx, &S->d_data, &S->data_cap, (size_t)ns * 2048)) return rc;
      if (int rc = efm_grow(ctx, &S->d_recs, &S->recs_cap, (size_t)ns)) return rc;
      LDG_LAUNCH_ON(st, "efmsec_sectors_write", ldg_k_efmsec_sectors<true>, dim3((unsigned)ft), 256, S->d_conf, nconf, w,
                    (int32_t*)nullptr, S->d_off[0], S->d_starts, S->d_counters);
      LDG_LAUNCH_ON(st, "efmsec_fix", ldg_k_efmsec_fix, dim3((unsigned)ns), FIX_THREADS, by, er, pos0, S->d_starts, S->d_gf,
                    S->d_scr, S->d_xp, S->d_sectors, S->d_data, S->d_recs, S->d_counters);
      if (int rc = check_launch(ctx, "ldg_k_efmsec_fix")) return rc;
    }
  }
  unsigned long long k[K_COUNT];
  LDG_TRY(hipMemcpyAsync(k, S->d_counters, sizeof(k), hipMemcpyDeviceToHost, st));
  LDG_TRY(hipStreamSynchronize(st));
  prof_collect(ctx);

  *info = ldg_efmsec_info{};
  info->first_byte = pos0 + held;
  info->bytes = n;
  info->first_sector = S->nsec;
  info->sectors = ns;
  info->candidates = g.candidates;
  info->confirmed = g.confirmed;
  info->coasted = (int64_t)k[K_COASTED];
  info->breaks = (int64_t)k[K_BREAKS] + advance(&S->carry, g);
  info->good = (int64_t)k[K_GOOD];
  info->corrected = (int64_t)k[K_CORRECTED];
  info->bad = (int64_t)k[K_BAD];
  info->other = (int64_t)k[K_OTHER];
  info->p_fixed = (int64_t)k[K_P_FIXED];
  info->q_fixed = (int64_t)k[K_Q_FIXED];
  info->erased_bytes = (int64_t)k[K_ERASED];
  S->cur = nxt;
  S->last_new_at = held;
  S->last_new = n;
  S->last_sectors = ns;
  S->off = g.tail_pos - pos0;
  S->held = nb - S->off;
  S->nsec += ns;
  S->ended = fin;
  info->held_bytes = S->held;
  S->last = *info;
  return LDG_OK;
}

}  // namespace

// ldg_efmdec_feed's hand-over: the bytes of local C2 rows [first, first + nbytes / 24)
static int efmsec_take(ldg_ctx* ctx, const uint8_t* c2, const uint32_t* c2f, int64_t first, int64_t nbytes, bool fin) {
  ldg_efmsec_info info;
  return efmsec_run(ctx, ctx->efmsec, nullptr, nullptr, c2, c2f, first, nbytes, fin, &info);
}

extern "C" {

int ldg_efmsec_enable(ldg_ctx* ctx, int on) {
  if (!ctx) return LDG_EINVAL;
  ldg_efmsec_state* S = nullptr;
  if (int rc = efmsec_state(ctx, &S)) return rc;
  LDG_TRY(hipStreamSynchronize(S->st));
  S->enabled = on != 0;
  efmsec_restart(ctx);
  return LDG_OK;
}

int ldg_efmsec_reset(ldg_ctx* ctx) {
  if (!ctx) return LDG_EINVAL;
  ldg_efmsec_state* S = nullptr;
  if (int rc = efmsec_state(ctx, &S)) return rc;
  efmsec_restart(ctx);
  return LDG_OK;
}

int ldg_efmsec_feed(ldg_ctx* ctx, const uint8_t* bytes, const uint8_t* erased, int64_t n, int final_, ldg_efmsec_info* info) {
  if (!ctx) return LDG_EINVAL;
  if (!info || n < 0 || (n > 0 && (!bytes || !erased))) {
    ctx->err = "ldg_efmsec_feed: bytes, erased and info are required";
    return LDG_EINVAL;
  }
  ldg_efmsec_state* S = nullptr;
  if (int rc = efmsec_state(ctx, &S)) return rc;
  return efmsec_run(ctx, S, bytes, erased, nullptr, nullptr, 0, n, final_ != 0, info);
}

int ldg_efmsec_last_info(ldg_ctx* ctx, ldg_efmsec_info* info) {
  if (!ctx || !info) return LDG_EINVAL;
  if (!ctx->efmsec) {
    ctx->err = "ldg_efmsec_last_info: the sector stage has not been used";
    return LDG_ESTATE;
  }
  *info = ctx->efmsec->last;
  return LDG_OK;
}

int64_t ldg_efmsec_read(ldg_ctx* ctx, int what, void* dst, int64_t cap) {
  if (!ctx || !dst || cap < 0 || !ctx->efmsec) return LDG_EINVAL;
  ldg_efmsec_state* S = ctx->efmsec;
  const void* src = nullptr;
  int64_t bytes = 0;
  const int64_t ns = S->last_sectors;
  switch (what) {
    case LDG_EFMSEC_DATA:    src = S->d_data;    bytes = ns * 2048; break;
    case LDG_EFMSEC_SECTORS: src = S->d_sectors; bytes = ns * ldg::efmsec::SECTOR; break;
    case LDG_EFMSEC_RECORDS: src = S->d_recs;    bytes = ns * (int64_t)sizeof(ldg_efmsec_rec); break;
    case LDG_EFMSEC_STARTS:  src = S->d_starts;  bytes = ns * 8; break;
    case LDG_EFMSEC_BYTES:   src = S->d_by[S->cur] ? S->d_by[S->cur] + S->last_new_at : nullptr; bytes = S->last_new; break;
    case LDG_EFMSEC_ERASED:  src = S->d_er[S->cur] ? S->d_er[S->cur] + S->last_new_at : nullptr; bytes = S->last_new; break;
    default: return LDG_EINVAL;
  }
  if (bytes > cap) bytes = cap;
  if (bytes == 0 || !src) return 0;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(S->st) != hipSuccess) return LDG_EDEVICE;
  if (hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) return LDG_EDEVICE;
  return bytes;
}

}  // extern "C"
