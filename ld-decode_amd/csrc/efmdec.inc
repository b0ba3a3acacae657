// Host side of the EFM decode (efmdec.hip; build-defined, DESIGN.md section 7d):
// ldg_efmdec_* of include/ldgpu.h.  Unity-built after efm.inc (efm_grow is its).

// efmsec.inc: the data-sector stage, fed each call's frames on the device when it is enabled
static bool efmsec_enabled(ldg_ctx* ctx);
static void efmsec_restart(ldg_ctx* ctx);
static int efmsec_take(ldg_ctx* ctx, const uint8_t* c2, const uint32_t* c2f, int64_t first, int64_t nbytes, bool fin);

struct ldg_efmdec_state {
  bool have_table = false;
  hipStream_t st = nullptr;
  uint16_t* d_inv = nullptr;
  uint8_t* d_gf = nullptr;
  unsigned long long* d_counters = nullptr;
  ldg::efmdec::GridOut* d_grid = nullptr;
  int64_t* d_tot = nullptr;                               // a scan's total
  // the stream between calls (efmdec_plan.hpp)
  ldg::efmdec::SyncCarry sync;
  ldg::efmdec::CircCarry circ;
  std::vector<uint8_t> tail;                              // run lengths the next call sees again
  bool ended = false;
  // grown on demand, never shrunk
  uint8_t* d_rl = nullptr;       size_t rl_cap = 0;
  int64_t* d_pos = nullptr;      size_t pos_cap = 0;
  int64_t* d_cand = nullptr;     size_t cand_cap = 0;
  int64_t* d_conf = nullptr;     size_t conf_cap = 0;
  int64_t* d_starts = nullptr;   size_t starts_cap = 0;
  int32_t* d_cnt[2] = {nullptr, nullptr};  size_t cnt_cap[2] = {0, 0};   // tiles' counts
  int64_t* d_off[2] = {nullptr, nullptr};  size_t off_cap[2] = {0, 0};   // and offsets
  uint8_t* d_f3[2] = {nullptr, nullptr};   size_t f3_cap[2] = {0, 0};    // held + fresh frames; the other: last call's
  int cur = 0;
  uint16_t* d_sub = nullptr;     size_t sub_cap = 0;
  uint8_t* d_c1 = nullptr;       size_t c1_cap = 0;
  uint8_t* d_c1f = nullptr;      size_t c1f_cap = 0;
  uint8_t* d_c2 = nullptr;       size_t c2_cap = 0;
  uint32_t* d_c2f = nullptr;     size_t c2f_cap = 0;
  int16_t* d_raw = nullptr;      size_t raw_cap = 0;
  uint8_t* d_rawf = nullptr;     size_t rawf_cap = 0;
  int16_t* d_pcm = nullptr;      size_t pcm_cap = 0;
  uint8_t* d_flg = nullptr;      size_t flg_cap = 0;
  // the last call, for ldg_efmdec_read
  int64_t last_held = 0, last_fresh = 0, last_first_frame = 0, last_elems = 0, last_first_sample = 0;
};

static void efmdec_free(ldg_ctx* ctx) {
  ldg_efmdec_state* D = ctx->efmdec;
  if (!D) return;
  if (D->st) {
    (void)hipStreamSynchronize(D->st);
    (void)hipStreamDestroy(D->st);
  }
  for (void* p : {(void*)D->d_inv, (void*)D->d_gf, (void*)D->d_counters, (void*)D->d_grid, (void*)D->d_tot, (void*)D->d_rl,
                  (void*)D->d_pos, (void*)D->d_cand, (void*)D->d_conf, (void*)D->d_starts, (void*)D->d_cnt[0],
                  (void*)D->d_cnt[1], (void*)D->d_off[0], (void*)D->d_off[1], (void*)D->d_f3[0], (void*)D->d_f3[1],
                  (void*)D->d_sub, (void*)D->d_c1, (void*)D->d_c1f, (void*)D->d_c2, (void*)D->d_c2f, (void*)D->d_raw,
                  (void*)D->d_rawf, (void*)D->d_pcm, (void*)D->d_flg})
    dfree(p);
  delete D;
  ctx->efmdec = nullptr;
}

namespace {

// count / scan / write: room for `tiles` counts and offsets in pair `which`
int efmdec_tiles(ldg_ctx* ctx, ldg_efmdec_state* D, int which, size_t tiles) {
  if (int rc = efm_grow(ctx, &D->d_cnt[which], &D->cnt_cap[which], tiles)) return rc;
  return efm_grow(ctx, &D->d_off[which], &D->off_cap[which], tiles);
}

int efmdec_total(ldg_ctx* ctx, ldg_efmdec_state* D, int64_t* out) {
  LDG_TRY(hipMemcpyAsync(out, D->d_tot, sizeof(int64_t), hipMemcpyDeviceToHost, D->st));
  LDG_TRY(hipStreamSynchronize(D->st));
  return LDG_OK;
}

}  // namespace

extern "C" {

int ldg_efmdec_set_table(ldg_ctx* ctx, const uint16_t* inverse, int n) {
  using namespace ldg::efmdec;
  if (!ctx) return LDG_EINVAL;
  auto bad = [&](const char* what) {
    ctx->err = std::string("ldg_efmdec_set_table: ") + what;
    return LDG_EINVAL;
  };
  if (!inverse || n != 1 << 14) return bad("the inverse table has 16384 entries");
  for (int i = 0; i < n; i++)
    if (inverse[i] > 0x101 && inverse[i] != 0xFFFF) return bad("an entry is neither a value, S0, S1 nor 0xFFFF");
  LDG_TRY(hipSetDevice(ctx->device));
  if (!ctx->efmdec) ctx->efmdec = new ldg_efmdec_state();
  ldg_efmdec_state* D = ctx->efmdec;
  if (!D->st && hipStreamCreateWithFlags(&D->st, hipStreamNonBlocking) != hipSuccess) {
    D->st = nullptr;
    ctx->err = "EFM decode: hipStreamCreate failed";
    return LDG_EDEVICE;
  }
  LDG_TRY(hipStreamSynchronize(D->st));
  if (!D->d_inv) {
    if (int rc = dmalloc(ctx, &D->d_inv, (size_t)n)) return rc;
    if (int rc = dmalloc(ctx, &D->d_gf, (size_t)GF_BYTES)) return rc;
    if (int rc = dmalloc(ctx, &D->d_counters, (size_t)K_COUNT)) return rc;
    if (int rc = dmalloc(ctx, &D->d_grid, 1)) return rc;
    if (int rc = dmalloc(ctx, &D->d_tot, 1)) return rc;
  }
  uint8_t gf[GF_BYTES] = {0};       // antilog, doubled, then log: polynomial 0x11d, alpha = 2
  unsigned x = 1;
  for (int i = 0; i < 255; i++) {
    gf[i] = gf[i + 255] = (uint8_t)x;
    gf[512 + x] = (uint8_t)i;
    x <<= 1;
    if (x & 0x100) x ^= 0x11d;
  }
  gf[510] = gf[0];
  gf[511] = gf[1];
  LDG_TRY(hipMemcpy(D->d_inv, inverse, (size_t)n * sizeof(uint16_t), hipMemcpyHostToDevice));
  LDG_TRY(hipMemcpy(D->d_gf, gf, sizeof(gf), hipMemcpyHostToDevice));
  D->have_table = true;
  return ldg_efmdec_reset(ctx);
}

int ldg_efmdec_reset(ldg_ctx* ctx) {
  if (!ctx) return LDG_EINVAL;
  ldg_efmdec_state* D = ctx->efmdec;
  if (!D || !D->have_table) {
    ctx->err = "ldg_efmdec_reset: ldg_efmdec_set_table has not been called";
    return LDG_ESTATE;
  }
  D->sync = ldg::efmdec::SyncCarry();
  D->circ = ldg::efmdec::CircCarry();
  D->tail.clear();
  D->ended = false;
  D->last_held = D->last_fresh = D->last_first_frame = D->last_elems = D->last_first_sample = 0;
  efmsec_restart(ctx);
  return LDG_OK;
}

int ldg_efmdec_feed(ldg_ctx* ctx, const uint8_t* rl, int64_t n, int final_, ldg_efmdec_info* info) {
  using namespace ldg::efmdec;
  if (!ctx) return LDG_EINVAL;
  auto bad = [&](const char* what) {
    ctx->err = std::string("ldg_efmdec_feed: ") + what;
    return LDG_EINVAL;
  };
  ldg_efmdec_state* D = ctx->efmdec;
  if (!D || !D->have_table) {
    ctx->err = "ldg_efmdec_feed: ldg_efmdec_set_table has not been called";
    return LDG_ESTATE;
  }
  if (D->ended) {
    ctx->err = "ldg_efmdec_feed: the stream has ended (ldg_efmdec_reset starts another)";
    return LDG_ESTATE;
  }
  if (!info || n < 0 || (n > 0 && !rl)) return bad("rl and info are required");
  if ((int64_t)D->tail.size() + n > ((int64_t)1 << 31) - 4096) return bad("at most 2^31 run lengths held in a call");
  LDG_TRY(hipSetDevice(ctx->device));
  hipStream_t st = D->st;
  *info = ldg_efmdec_info{};
  const bool fin = final_ != 0;

  // ---- the frame grid over the held run lengths and the new ones ----
  D->tail.insert(D->tail.end(), rl, rl + n);
  const int64_t nrun = (int64_t)D->tail.size();
  LDG_TRY(hipMemsetAsync(D->d_counters, 0, K_COUNT * sizeof(unsigned long long), st));
  int64_t ncand = 0, nconf = 0, fresh = 0;
  GridOut g{D->sync.pos0, fin ? NEVER : std::max(D->sync.emit_from, D->sync.pos0 - SETTLE + 1), 0, D->sync.pos0, 0, 0, 0};
  if (nrun > 0) {
    const int64_t rt = (nrun + RUN_TILE - 1) / RUN_TILE;
    if (int rc = efm_grow(ctx, &D->d_rl, &D->rl_cap, (size_t)nrun)) return rc;
    if (int rc = efm_grow(ctx, &D->d_pos, &D->pos_cap, (size_t)nrun + 1)) return rc;
    // the pairs also hold the candidates' and the confirmed candidates' tiles of 256 (fewer than nrun)
    if (int rc = efmdec_tiles(ctx, D, 0, (size_t)(nrun / 256 + 1))) return rc;
    if (int rc = efmdec_tiles(ctx, D, 1, (size_t)(nrun / 256 + 1))) return rc;
    LDG_TRY(hipMemcpyAsync(D->d_rl, D->tail.data(), (size_t)nrun, hipMemcpyHostToDevice, st));
    LDG_LAUNCH_ON(st, "efmdec_runsum", ldg_k_efmdec_runsum, dim3((unsigned)rt), 256, D->d_rl, nrun, D->d_cnt[0]);
    LDG_LAUNCH_ON(st, "efmdec_scan", ldg::efm::ldg_k_efm_scan, dim3(1), 1024, D->d_cnt[0], rt, D->d_off[0], D->d_tot);
    LDG_LAUNCH_ON(st, "efmdec_cand_count", ldg_k_efmdec_cand<false>, dim3((unsigned)rt), 256, D->d_rl, nrun, D->sync.pos0,
                  D->d_off[0], D->d_pos, D->d_cnt[1], (const int64_t*)nullptr, (int64_t*)nullptr);
    LDG_LAUNCH_ON(st, "efmdec_scan", ldg::efm::ldg_k_efm_scan, dim3(1), 1024, D->d_cnt[1], rt, D->d_off[1], D->d_tot);
    if (int rc = check_launch(ctx, "ldg_k_efmdec_cand")) return rc;
    if (int rc = efmdec_total(ctx, D, &ncand)) return rc;
    if (int rc = efm_grow(ctx, &D->d_cand, &D->cand_cap, (size_t)ncand + 1)) return rc;
    if (int rc = efm_grow(ctx, &D->d_conf, &D->conf_cap, (size_t)ncand + 1)) return rc;
    if (ncand > 0) {
      LDG_LAUNCH_ON(st, "efmdec_cand_write", ldg_k_efmdec_cand<true>, dim3((unsigned)rt), 256, D->d_rl, nrun, D->sync.pos0,
                    D->d_off[0], D->d_pos, (int32_t*)nullptr, D->d_off[1], D->d_cand);
      const int64_t ct = (ncand + 255) / 256;
      LDG_LAUNCH_ON(st, "efmdec_confirm_count", ldg_k_efmdec_confirm<false>, dim3((unsigned)ct), 256, D->d_cand, ncand,
                    D->d_cnt[0], (const int64_t*)nullptr, (int64_t*)nullptr);
      LDG_LAUNCH_ON(st, "efmdec_scan", ldg::efm::ldg_k_efm_scan, dim3(1), 1024, D->d_cnt[0], ct, D->d_off[0], D->d_tot);
      LDG_LAUNCH_ON(st, "efmdec_confirm_write", ldg_k_efmdec_confirm<true>, dim3((unsigned)ct), 256, D->d_cand, ncand,
                    (int32_t*)nullptr, D->d_off[0], D->d_conf);
      if (int rc = check_launch(ctx, "ldg_k_efmdec_confirm")) return rc;
      if (int rc = efmdec_total(ctx, D, &nconf)) return rc;
    }
    const int64_t ft = (nconf + 255) / 256;
    if (nconf > 0) {
      LDG_LAUNCH_ON(st, "efmdec_frames_count", ldg_k_efmdec_frames<false>, dim3((unsigned)ft), 256, D->d_conf, nconf,
                    D->d_pos + nrun, D->sync.emit_from, fin ? 1 : 0, D->d_cnt[1], (const int64_t*)nullptr, (int64_t*)nullptr,
                    D->d_counters);
      LDG_LAUNCH_ON(st, "efmdec_scan", ldg::efm::ldg_k_efm_scan, dim3(1), 1024, D->d_cnt[1], ft, D->d_off[1], D->d_tot);
    }
    LDG_LAUNCH_ON(st, "efmdec_finish", ldg_k_efmdec_finish, dim3(1), 64, D->d_pos, nrun, D->d_cand, ncand, D->d_conf, nconf,
                  D->sync.emit_from, fin ? 1 : 0, D->d_grid);
    if (int rc = check_launch(ctx, "ldg_k_efmdec_frames")) return rc;
    LDG_TRY(hipMemcpyAsync(&g, D->d_grid, sizeof(g), hipMemcpyDeviceToHost, st));
    if (nconf > 0) {
      if (int rc = efmdec_total(ctx, D, &fresh)) return rc;
    } else {
      LDG_TRY(hipStreamSynchronize(st));
    }
  }

  // ---- symbols, CIRC and samples over the held frames and the fresh ones ----
  const CircPlan P = circ_plan(D->circ, fresh, fin);
  const int64_t held = D->circ.held, total = P.total;
  const int64_t nraw = total > LATENCY ? (total - LATENCY) * 12 : 0;
  const int64_t elems = (P.e1 - D->circ.e0) * 12;                        // samples x channels out
  const int64_t first_raw = (D->circ.e0 - D->circ.g0 - LATENCY) * 12;
  const int nxt = D->cur ^ 1;
  if (total > 0) {
    if (int rc = efm_grow(ctx, &D->d_f3[nxt], &D->f3_cap[nxt], (size_t)total * 32)) return rc;
    if (int rc = efm_grow(ctx, &D->d_c1, &D->c1_cap, (size_t)total * 28)) return rc;
    if (int rc = efm_grow(ctx, &D->d_c1f, &D->c1f_cap, (size_t)total)) return rc;
    if (int rc = efm_grow(ctx, &D->d_c2, &D->c2_cap, (size_t)total * 28)) return rc;
    if (int rc = efm_grow(ctx, &D->d_c2f, &D->c2f_cap, (size_t)total)) return rc;
    if (int rc = efm_grow(ctx, &D->d_sub, &D->sub_cap, (size_t)fresh + 1)) return rc;
    if (int rc = efm_grow(ctx, &D->d_starts, &D->starts_cap, (size_t)fresh + 1)) return rc;
    if (int rc = efm_grow(ctx, &D->d_raw, &D->raw_cap, (size_t)nraw + 1)) return rc;
    if (int rc = efm_grow(ctx, &D->d_rawf, &D->rawf_cap, (size_t)nraw + 1)) return rc;
    if (int rc = efm_grow(ctx, &D->d_pcm, &D->pcm_cap, (size_t)elems + 1)) return rc;
    if (int rc = efm_grow(ctx, &D->d_flg, &D->flg_cap, (size_t)elems + 1)) return rc;
    // rows no kernel writes (no C1 for local frame 0, no C2 below 109) read as zeros
    LDG_TRY(hipMemsetAsync(D->d_c1, 0, (size_t)total * 28, st));
    LDG_TRY(hipMemsetAsync(D->d_c1f, 0, (size_t)total, st));
    LDG_TRY(hipMemsetAsync(D->d_c2, 0, (size_t)total * 28, st));
    LDG_TRY(hipMemsetAsync(D->d_c2f, 0, (size_t)total * sizeof(uint32_t), st));
    if (held > 0)
      LDG_TRY(hipMemcpyAsync(D->d_f3[nxt], D->d_f3[D->cur] + (size_t)(D->last_held + D->last_fresh - held) * 32,
                             (size_t)held * 32, hipMemcpyDeviceToDevice, st));
    if (fresh > 0) {
      const int64_t ft = (nconf + 255) / 256;
      LDG_LAUNCH_ON(st, "efmdec_frames_write", ldg_k_efmdec_frames<true>, dim3((unsigned)ft), 256, D->d_conf, nconf,
                    D->d_pos + nrun, D->sync.emit_from, fin ? 1 : 0, (int32_t*)nullptr, D->d_off[1], D->d_starts,
                    D->d_counters);
      LDG_LAUNCH_ON(st, "efmdec_symbols", ldg_k_efmdec_symbols, dim3((unsigned)((fresh + SYM_FRAMES - 1) / SYM_FRAMES)),
                    64 * SYM_FRAMES, D->d_pos, nrun + 1, D->d_starts, fresh, D->d_inv, D->d_sub, D->d_f3[nxt] + (size_t)held * 32,
                    D->d_counters);
    }
    if (total > 1)
      LDG_LAUNCH_ON(st, "efmdec_c1", ldg_k_efmdec_c1, dim3((unsigned)((total - 1 + 255) / 256)), 256, D->d_f3[nxt], total,
                    D->d_gf, std::max<int64_t>(held, 1), D->d_c1, D->d_c1f, D->d_counters);
    if (total > C2_FIRST)
      LDG_LAUNCH_ON(st, "efmdec_c2", ldg_k_efmdec_c2, dim3((unsigned)((total - C2_FIRST + 255) / 256)), 256, D->d_c1, D->d_c1f,
                    total, D->d_gf, std::max<int64_t>(held, C2_FIRST), D->d_c2, D->d_c2f, D->d_counters);
    if (nraw > 0)
      LDG_LAUNCH_ON(st, "efmdec_pcm", ldg_k_efmdec_pcm, dim3((unsigned)((nraw + 255) / 256)), 256, D->d_c2, D->d_c2f, total,
                    D->d_raw, D->d_rawf);
    if (elems > 0)
      LDG_LAUNCH_ON(st, "efmdec_conceal", ldg_k_efmdec_conceal, dim3((unsigned)((elems + 255) / 256)), 256, D->d_raw, D->d_rawf,
                    nraw, first_raw, elems, D->d_pcm, D->d_flg, D->d_counters);
    if (int rc = check_launch(ctx, "ldg_k_efmdec_*")) return rc;
    D->cur = nxt;
  }
  unsigned long long k[K_COUNT];
  LDG_TRY(hipMemcpyAsync(k, D->d_counters, sizeof(k), hipMemcpyDeviceToHost, st));
  LDG_TRY(hipStreamSynchronize(st));
  prof_collect(ctx);

  info->first_frame = D->circ.g0 + held;
  info->frames = fresh;
  info->first_sample = (D->circ.e0 - LATENCY) * 6;
  info->samples = elems / 12 * 6;
  info->candidates = g.candidates;
  info->confirmed = g.confirmed;
  info->coasted = (int64_t)k[K_COASTED];
  info->breaks = (int64_t)k[K_BREAKS] + advance(&D->sync, g);
  info->bad_symbols = (int64_t)k[K_BAD];
  info->c1_pass = (int64_t)k[K_C1_PASS];
  info->c1_fixed = (int64_t)k[K_C1_FIXED];
  info->c1_erased = (int64_t)k[K_C1_ERASED];
  info->c2_pass = (int64_t)k[K_C2_PASS];
  info->c2_fixed = (int64_t)k[K_C2_FIXED];
  info->c2_erasure_solved = (int64_t)k[K_C2_SOLVED];
  info->c2_failed = (int64_t)k[K_C2_FAILED];
  info->c2_unsolved = (int64_t)k[K_C2_UNSOLVED];
  info->flagged = (int64_t)k[K_FLAGGED];
  info->averaged = (int64_t)k[K_AVERAGED];
  info->muted = (int64_t)k[K_MUTED];
  D->last_held = held;
  D->last_fresh = fresh;
  D->last_first_frame = info->first_frame;
  D->last_elems = elems;
  D->last_first_sample = info->first_sample;
  // the same frames' bytes, before concealment, to the sector stage (24 a frame: two a value)
  if (efmsec_enabled(ctx))
    if (int rc = efmsec_take(ctx, D->d_c2, D->d_c2f, D->circ.e0 - D->circ.g0, elems * 2, fin)) return rc;
  circ_advance(&D->circ, P);
  D->tail.erase(D->tail.begin(), D->tail.begin() + (size_t)g.tail_idx);
  info->held_runs = (int64_t)D->tail.size();
  D->ended = fin;
  return LDG_OK;
}

int64_t ldg_efmdec_read(ldg_ctx* ctx, int what, void* dst, int64_t cap, int64_t* first) {
  if (!ctx || !dst || cap < 0 || !ctx->efmdec) return LDG_EINVAL;
  ldg_efmdec_state* D = ctx->efmdec;
  const void* src = nullptr;
  int64_t bytes = 0, at = D->last_first_frame;
  const size_t h = (size_t)D->last_held;
  const int64_t f = D->last_fresh;
  switch (what) {
    case LDG_EFMDEC_PCM:      src = D->d_pcm;                    bytes = D->last_elems * 2;  at = D->last_first_sample; break;
    case LDG_EFMDEC_FLAGS:    src = D->d_flg;                    bytes = D->last_elems;      at = D->last_first_sample; break;
    case LDG_EFMDEC_SUBCODE:  src = D->d_sub;                    bytes = f * 2;  break;
    case LDG_EFMDEC_STARTS:   src = D->d_starts;                 bytes = f * 8;  break;
    case LDG_EFMDEC_F3:       src = D->d_f3[D->cur] ? D->d_f3[D->cur] + h * 32 : nullptr;  bytes = f * 32; break;
    case LDG_EFMDEC_C1:       src = D->d_c1 ? D->d_c1 + h * 28 : nullptr;   bytes = f * 28; break;
    case LDG_EFMDEC_C1_FLAGS: src = D->d_c1f ? D->d_c1f + h : nullptr;      bytes = f;      break;
    case LDG_EFMDEC_C2:       src = D->d_c2 ? D->d_c2 + h * 28 : nullptr;   bytes = f * 28; break;
    case LDG_EFMDEC_C2_FLAGS: src = D->d_c2f ? D->d_c2f + h : nullptr;      bytes = f * 4;  break;
    default: return LDG_EINVAL;
  }
  if (first) *first = at;
  if (bytes > cap) bytes = cap;
  if (bytes == 0 || !src) return 0;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(D->st) != hipSuccess) return LDG_EDEVICE;
  if (hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) return LDG_EDEVICE;
  return bytes;
}

}  // extern "C"
