// Host side of the C ABI, unit: agp_remove_data — remove_data! of the reference (src/api.jl:449-468) on the resident series and the
// resident factors.  The series is compacted and uploaded again through agp_set_data's own body (same grid / lattice detection, same
// tables); every factor the store holds on a prefix that contains removed positions is UPDATED to the factor of the reduced prefix
// (csrc/agp_remove_kernel.hpp: a rank-r update of the trailing triangle per removed run, on the new tile grid) or dropped where
// remove_admits says refactoring is cheaper.  Keys stay (program, parameters, noise); only the stored prefix length changes, so the
// next agp_logpdf_batch_extend at the new n — the reference's smc_step! after deleteat! — hits the updated factors.
#include "agp_host.hpp"
#include "agp_remove_kernel.hpp"

#include <map>

namespace {

struct Run { int64_t a, r; };      // positions [a, a + r) of the series AS IT IS when the run's turn comes (earlier runs already gone)

// the removed positions below n_f as runs, first to last, each in the coordinates left by the runs before it
std::vector<Run> runs_below(const int64_t* idx, int64_t cnt) {
  std::vector<Run> runs;
  int64_t gone = 0;
  for (int64_t i = 0; i < cnt;) {
    int64_t j = i + 1;
    while (j < cnt && idx[j] == idx[j - 1] + 1) ++j;
    runs.push_back({idx[i] - gone, j - i});
    gone += j - i;
    i = j;
  }
  return runs;
}

template <int RH> void launch_panel(hipStream_t st, int Pc, const RemoveArgs& g) { hipLaunchKernelGGL(k_rm_panel<RH>, dim3(Pc), dim3(320), 0, st, g); }
template <int RH> void launch_apply(hipStream_t st, int nI, int Pc, const RemoveArgs& g) { hipLaunchKernelGGL(k_rm_apply<RH>, dim3(nI, Pc), dim3(256), 0, st, g); }

// The slot-indexed arrays an update rewrites: the factor store's (remove_body) or a probe's own (agp_debug_remove_factor).
struct FactorView {
  double* A; long long strideA;
  double* Winv; int wsteps;
  double* vec; int ldv;
  double* partial; int ntp;
  int* info;
};

// One run out of the factors (prefix n_old) of the chunk's slots.  Returns the panel steps launched in *panels.
hipError_t remove_run(agp_ctx* c, Slot* s, hipStream_t st, const FactorView& fv, const int32_t* d_slot, int Pc, int64_t n_old, const Run& run, int64_t* panels) {
  const int64_t n_new = n_old - run.r;
  const int nt_new = round_up(n_new, NB) / NB, J0 = (int)(run.a / NB);
  if (J0 >= nt_new) return hipSuccess;      // a whole number of trailing tile rows went: what stays is the factor as it is
  RemoveArgs g = {};
  g.A = fv.A; g.strideA = fv.strideA; g.Winv = fv.Winv; g.wsteps = fv.wsteps;
  g.vec = fv.vec; g.ldv = fv.ldv; g.partial = fv.partial; g.ntp = fv.ntp;
  g.info = fv.info; g.slot = d_slot;
  g.off0 = tile_off(J0, 0); g.ws_stride = tile_off(nt_new, 0) - g.off0;
  g.ldw = nt_new * NB; g.ldg = (int)run.r;
  g.a = (int)run.a; g.r = (int)run.r; g.n_new = (int)n_new; g.nt_new = nt_new; g.J0 = J0;
  hipError_t e;
  if ((e = s->A.ensure(sizeof(double) * (size_t)g.ws_stride * Pc)) != hipSuccess) return e;
  if ((e = s->W.ensure(sizeof(double) * (size_t)RM_RMAX * g.ldw * Pc)) != hipSuccess) return e;
  if ((e = s->alpha.ensure(sizeof(double) * (size_t)g.ldg * Pc)) != hipSuccess) return e;
  if ((e = s->Z.ensure(sizeof(double) * (size_t)RM_VSTRIDE * Pc)) != hipSuccess) return e;
  g.ws = s->A.as<double>(); g.Wk = s->W.as<double>(); g.G = s->alpha.as<double>(); g.V = s->Z.as<double>();
  if (c->poison.active()) {
    // NaN-poison mode: the destination rows read NaN until the update writes them, like the rows an extension sweep recomputes
    const size_t bytes = sizeof(double) * (size_t)g.ws_stride * Pc;
    if ((e = hipMemsetAsync(g.ws, POISON_BYTE, bytes, st)) != hipSuccess) return e;
    c->poison.count(bytes);
  }
  for (int c0 = 0; c0 < g.r; c0 += RM_RMAX) {
    g.c0 = c0; g.rc = std::min(RM_RMAX, g.r - c0);
    g.first = c0 == 0; g.last = c0 + g.rc == g.r;
    hipLaunchKernelGGL(k_rm_init, dim3(nt_new - J0, Pc), dim3(256), 0, st, g);
    if (g.first && J0 > 0) hipLaunchKernelGGL(k_rm_copy, dim3(J0 * (nt_new - J0), Pc), dim3(256), 0, st, g);
    for (int J = J0; J < nt_new; ++J) {
      g.J = J;
      const int nI = nt_new - J - 1;
      if (g.rc <= 2) { launch_panel<1>(st, Pc, g); if (nI > 0) launch_apply<1>(st, nI, Pc, g); }
      else if (g.rc <= 8) { launch_panel<4>(st, Pc, g); if (nI > 0) launch_apply<4>(st, nI, Pc, g); }
      else { launch_panel<16>(st, Pc, g); if (nI > 0) launch_apply<16>(st, nI, Pc, g); }
      ++*panels;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const int gx = (int)std::max<long long>(1, std::min<long long>(1024, g.ws_stride / 512));
  hipLaunchKernelGGL(k_rm_commit, dim3(gx, Pc), dim3(256), 0, st, g);
  return hipGetLastError();
}

int remove_body(agp_ctx* c, const int64_t* idx, int64_t k) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (!c->d_ts || c->n_max <= 0) return fail(c, AGP_ERR_NODATA, "agp_remove_data before agp_set_data");
  if (!idx || k <= 0) return fail(c, AGP_ERR_ARG, "no such time points: an empty list of positions");
  for (int64_t i = 0; i < k; ++i) {
    if (idx[i] < 0 || idx[i] >= c->n_max) return fail(c, AGP_ERR_ARG, "no such time points: position out of range");
    if (i > 0 && idx[i] <= idx[i - 1]) return fail(c, AGP_ERR_ARG, "positions must be distinct and ascending");
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  const int64_t n_old = c->n_max, n_new = n_old - k;
  std::vector<double> ts((size_t)std::max<int64_t>(n_new, 1)), xs((size_t)std::max<int64_t>(n_new, 1));
  {
    int64_t o = 0, q = 0;
    for (int64_t i = 0; i < n_old; ++i) {
      if (q < k && idx[q] == i) { ++q; continue; }
      ts[(size_t)o] = c->h_ts[(size_t)i]; xs[(size_t)o] = c->h_xs[(size_t)i]; ++o;
    }
  }
  std::vector<uint8_t> touched;
  int64_t n_upd = 0, n_drop = 0, n_panels = 0;
  if (!c->ref_arith) {
    agp_ctx::FactorStore& fs = c->store;
    std::unique_lock<std::mutex> lk(fs.mu);
    touched.assign((size_t)fs.n_slots, 0);
    auto drop = [&](int sl) {
      if (!fs.key[(size_t)sl].empty()) fs.index.erase(fs.key[(size_t)sl]);
      fs.key[(size_t)sl].clear(); fs.n_cached[(size_t)sl] = 0; fs.zrows[(size_t)sl] = 0; fs.used[(size_t)sl] = 0;
      ++n_drop;
    };
    // factors by prefix length: each sees the removed positions below its own n_f
    std::map<int64_t, std::vector<int32_t>> groups;
    for (int sl = 0; sl < fs.n_slots; ++sl) {
      if (fs.key[(size_t)sl].empty()) continue;
      const int64_t n_f = fs.n_cached[(size_t)sl];
      const int64_t cnt = std::lower_bound(idx, idx + k, n_f) - idx;
      if (cnt == 0) continue;                                  // untouched: a prefix of the reduced series as it stands
      const int64_t t = n_f - cnt - idx[0];                    // rows of the trailing triangle from the first removed position on
      const int n_runs = (int)runs_below(idx, cnt).size();
      if (!c->remove_update || fs.info_h[(size_t)sl] != 0 || n_f - cnt <= 0 || !(c->remove_update >= 2 || remove_admits(t, cnt, n_runs))) { drop(sl); continue; }
      groups[n_f].push_back(sl);
    }
    if (!groups.empty()) {
      SlotGuard sg(c);
      Slot* s = sg.s;
      if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
      hipStream_t st = s->stream;
      auto forget_groups = [&]() { for (auto& gr : groups) for (int32_t sl : gr.second) if (!fs.key[(size_t)sl].empty()) drop(sl); };
      const FactorView fv = {fs.A.as<double>(), fs.strideA, fs.W.as<double>(), fs.nt_cap, fs.vec.as<double>(), fs.nt_cap * NB,
                             fs.partial.as<double>(), fs.nt_cap, fs.info.as<int>()};
      auto hipfail = [&](hipError_t e, const char* what) {
        forget_groups();
        return fail(c, AGP_ERR_HIP, std::string("HIP error in agp_remove_data (") + what + "): " + hipGetErrorString(e));
      };
#define RMCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hipfail(e_, #expr); } while (0)
      for (auto& gr : groups) {
        const int64_t n_f = gr.first;
        const std::vector<int32_t>& sl_all = gr.second;
        const int64_t cnt = std::lower_bound(idx, idx + k, n_f) - idx;
        const std::vector<Run> runs = runs_below(idx, cnt);
        // particles per chunk: the workspace holds the tile rows from the first touched one on
        const int nt_f = round_up(n_f, NB) / NB;
        const int64_t bytes_pp = (int64_t)sizeof(double) * (tile_off(nt_f, 0) + (int64_t)RM_RMAX * nt_f * NB + RM_VSTRIDE + cnt);
        const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)sl_all.size(), std::min<int64_t>(ws_limit_bytes(c), 16LL << 30) / bytes_pp));
        RMCHK(s->map.ensure(sizeof(int32_t) * (size_t)chunk));
        RMCHK(s->h_stage.ensure(sizeof(int32_t) * (size_t)chunk));
        for (size_t p0 = 0; p0 < sl_all.size(); p0 += (size_t)chunk) {
          const int Pc = (int)std::min<size_t>((size_t)chunk, sl_all.size() - p0);
          RMCHK(hipStreamSynchronize(st));            // (the pinned slot list is reused chunk by chunk)
          std::memcpy(s->h_stage.p, sl_all.data() + p0, sizeof(int32_t) * (size_t)Pc);
          RMCHK(hipMemcpyAsync(s->map.p, s->h_stage.p, sizeof(int32_t) * (size_t)Pc, hipMemcpyHostToDevice, st));
          int64_t n_cur = n_f;
          for (const Run& run : runs) {
            RMCHK(remove_run(c, s, st, fv, s->map.as<int32_t>(), Pc, n_cur, run, &n_panels));
            n_cur -= run.r;
          }
        }
      }
      // LAPACK info of the updated slots: a non-finite or non-positive new diagonal drops the slot (the next sweep factors it from
      // scratch and reports the particle's info there)
      RMCHK(s->h_out.ensure(sizeof(int32_t) * (size_t)fs.n_slots));
      RMCHK(hipMemcpyAsync(s->h_out.p, fs.info.p, sizeof(int32_t) * (size_t)fs.n_slots, hipMemcpyDeviceToHost, st));
      RMCHK(hipStreamSynchronize(st));
#undef RMCHK
      const int32_t* hinfo = static_cast<const int32_t*>(s->h_out.p);
      for (auto& gr : groups) {
        const int64_t cnt = std::lower_bound(idx, idx + k, gr.first) - idx;
        for (int32_t sl : gr.second) {
          if (hinfo[sl] != 0) { fs.info_h[(size_t)sl] = hinfo[sl]; drop(sl); continue; }
          fs.n_cached[(size_t)sl] = gr.first - cnt;
          fs.zrows[(size_t)sl] = 0;                 // the resident L^-T belongs to the old factor
          touched[(size_t)sl] = 1;
          ++n_upd;
        }
      }
    }
  }
  const int rc = set_data_after_remove(c, ts.data(), xs.data(), n_new, touched);
  {
    std::lock_guard<std::mutex> g(c->mu);
    c->rm_updated += n_upd; c->rm_dropped += n_drop; c->rm_rows += k; c->rm_panels += n_panels;
  }
  return rc;
}

// agp_debug_remove_factor: P caller factors packed into arrays of the store's layout (in slot buffers remove_run does not take as
// its workspace), every run of idx through remove_run as remove_body sends it, and what the kernels left, at the new size.
int debug_remove_body(agp_ctx* c, const double* L0, const double* alpha0, int64_t n, int32_t P, const int64_t* idx, int64_t k,
                      double* out_L, double* out_alpha, double* out_partial, double* out_winv, int32_t* out_info) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (!L0 || !idx || !out_L || !out_alpha || !out_partial || !out_info) return fail(c, AGP_ERR_ARG, "debug probe: null pointer");
  if (n < 2 || n > 1024 || P < 1 || k < 1 || k >= n) return fail(c, AGP_ERR_ARG, "debug probe: needs 2 <= n <= 1024, P >= 1, 1 <= k < n");
  if ((int64_t)P * n * n > ((int64_t)1 << 24)) return fail(c, AGP_ERR_ARG, "debug probe: batch too large");
  for (int64_t i = 0; i < k; ++i) {
    if (idx[i] < 0 || idx[i] >= n) return fail(c, AGP_ERR_ARG, "debug probe: position out of range");
    if (i > 0 && idx[i] <= idx[i - 1]) return fail(c, AGP_ERR_ARG, "positions must be distinct and ascending");
  }
  const int nt = round_up(n, NB) / NB;
  const long long strideA = tile_off(nt, 0);
  if ((int64_t)P * strideA > ((int64_t)1 << 27)) return fail(c, AGP_ERR_ARG, "debug probe: batch too large (padded tiles)");
  const int64_t n_new = n - k;
  const int nt_new = round_up(n_new, NB) / NB, np_new = nt_new * NB, ldv = nt * NB;
  const size_t nel = (size_t)n * n, nW = (size_t)P * nt * NSB * 256, nPart = (size_t)P * nt * 2;
  // the caller's lower triangles as launch_pack_dense reads them (element (r, c) at [c * n + r]); zero above the diagonal
  std::vector<double> Lt(nel * P, 0.0);
  for (int p = 0; p < P; ++p)
    for (int64_t r = 0; r < n; ++r)
      for (int64_t cc = 0; cc <= r; ++cc) Lt[p * nel + (size_t)cc * n + r] = L0[p * nel + (size_t)r * n + cc];
  HIPCHK(c, hipSetDevice(c->device));
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  // (remove_run's workspace is the slot's A, W, alpha and Z: the factor arrays live in dense, tsol, vec, partial, info)
  HIPCHK(c, s->pred_cov.ensure(sizeof(double) * nel * P));
  HIPCHK(c, s->dense.ensure(sizeof(double) * (size_t)strideA * P));
  HIPCHK(c, s->tsol.ensure(sizeof(double) * nW));
  HIPCHK(c, s->vec.ensure(sizeof(double) * (size_t)ldv * P));
  HIPCHK(c, s->partial.ensure(sizeof(double) * nPart));
  HIPCHK(c, s->info.ensure(sizeof(int) * (size_t)P));
  HIPCHK(c, s->map.ensure(sizeof(int32_t) * (size_t)P));
  const FactorView fv = {s->dense.as<double>(), strideA, s->tsol.as<double>(), nt, s->vec.as<double>(), ldv, s->partial.as<double>(), nt,
                         s->info.as<int>()};
  std::vector<double> sentinel(std::max(nW, nPart), -7.0);
  std::vector<int32_t> ident((size_t)P);
  for (int p = 0; p < P; ++p) ident[(size_t)p] = p;
  HIPCHK(c, hipMemcpyAsync(s->pred_cov.p, Lt.data(), sizeof(double) * nel * P, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(fv.Winv, sentinel.data(), sizeof(double) * nW, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(fv.partial, sentinel.data(), sizeof(double) * nPart, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(s->map.p, ident.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(fv.vec, 0, sizeof(double) * (size_t)ldv * P, st));
  if (alpha0)
    HIPCHK(c, hipMemcpy2DAsync(fv.vec, sizeof(double) * ldv, alpha0, sizeof(double) * n, sizeof(double) * n, P, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(fv.info, 0, sizeof(int) * (size_t)P, st));
  for (int p = 0; p < P; ++p)
    launch_pack_dense(st, s->pred_cov.as<double>() + (size_t)p * nel, (int)n, nt, strideA, fv.A + (size_t)p * strideA);
  HIPCHK(c, hipGetLastError());
  int64_t n_cur = n, panels = 0;
  for (const Run& run : runs_below(idx, k)) {
    HIPCHK(c, remove_run(c, s, st, fv, s->map.as<int32_t>(), P, n_cur, run, &panels));
    n_cur -= run.r;
  }
  std::vector<double> hA((size_t)strideA * P), hv((size_t)ldv * P), hp(nPart), hw(out_winv ? nW : 0);
  HIPCHK(c, hipMemcpyAsync(hA.data(), fv.A, sizeof(double) * hA.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(hv.data(), fv.vec, sizeof(double) * hv.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(hp.data(), fv.partial, sizeof(double) * nPart, hipMemcpyDeviceToHost, st));
  if (out_winv) HIPCHK(c, hipMemcpyAsync(hw.data(), fv.Winv, sizeof(double) * nW, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out_info, fv.info, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  // the padded new grid as it lies in the tiles: both triangles of the diagonal tiles, nothing (zero) where the layout has no tile
  for (int p = 0; p < P; ++p) {
    double* Lp = out_L + (size_t)p * np_new * np_new;
    const double* Ap = hA.data() + (size_t)p * strideA;
    for (int i = 0; i < np_new; ++i)
      for (int j = 0; j < np_new; ++j)
        Lp[(size_t)i * np_new + j] = (j >> 7) > (i >> 7) ? 0.0 : Ap[tile_off(i >> 7, j >> 7) + (long long)(j & 127) * NB + (i & 127)];
    std::memcpy(out_alpha + (size_t)p * np_new, hv.data() + (size_t)p * ldv, sizeof(double) * (size_t)np_new);
    std::memcpy(out_partial + (size_t)p * nt_new * 2, hp.data() + (size_t)p * nt * 2, sizeof(double) * (size_t)nt_new * 2);
    if (out_winv)
      std::memcpy(out_winv + (size_t)p * nt_new * NSB * 256, hw.data() + (size_t)p * nt * NSB * 256, sizeof(double) * (size_t)nt_new * NSB * 256);
  }
  return AGP_OK;
}

}  // namespace

extern "C" {

int agp_debug_remove_factor(agp_ctx* c, const double* L0, const double* alpha0, int64_t n, int32_t P, const int64_t* idx, int64_t k,
                            double* out_L, double* out_alpha, double* out_partial, double* out_winv, int32_t* out_info) {
  return abi_guard(c, [&] { return debug_remove_body(c, L0, alpha0, n, P, idx, k, out_L, out_alpha, out_partial, out_winv, out_info); });
}

int agp_remove_data(agp_ctx* c, const int64_t* idx, int64_t k) {
  return abi_guard(c, [&] { return remove_body(c, idx, k); });
}

int agp_remove_data_multi(agp_ctx* const* ctxs, int32_t n_dev, const int64_t* idx, int64_t k) {
  if (!ctxs || n_dev < 1) return fail(nullptr, AGP_ERR_ARG, "bad arguments");
  for (int i = 0; i < n_dev; ++i) {
    const int rc = agp_remove_data(ctxs[i], idx, k);
    if (rc) return rc;
  }
  return AGP_OK;
}

int agp_get_remove_stats(agp_ctx* c, int64_t* out, int32_t n_out) {
  if (!c || !out || n_out < 0) return fail(c, AGP_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> g(c->mu);
  const int64_t v[4] = {c->rm_updated, c->rm_dropped, c->rm_rows, c->rm_panels};
  for (int i = 0; i < n_out && i < 4; ++i) out[i] = v[i];
  return AGP_OK;
}

int agp_set_remove_update(agp_ctx* c, int32_t on) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  c->remove_update = on <= 0 ? 0 : on == 1 ? 1 : 2;      // (2: update whatever remove_admits says — tools/gpu_remove_perf.py measures the rule with it)
  return AGP_OK;
}

}  // extern "C"
