// Sanitizer harness for dolfinx_materials_amd/csrc/host_side.hpp (the GPU-free host code of libdxmat.so).
//
//   clang++ -std=c++17 -O1 -g -fsanitize=thread            host_side_harness.cpp -o harness_tsan
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined host_side_harness.cpp -o harness_asan
//   harness_* <input.bin> <output.bin>
//
// Built and run by tests/test_host_side_sanitizers.py (`-m "not gpu"`), which writes the input arrays, compares the rebuilt
// tangent blocks in <output.bin> with oracle/host_rebuild_np.py and fails on any sanitizer report.  The "GPU" of the chunk
// pipeline is played by plain memcpy on the calling thread; everything else is the code the product runs.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../dolfinx_materials_amd/csrc/host_side.hpp"

using namespace dxm_host;

static int g_failures = 0;
#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      ++g_failures;                                         \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);  \
      fprintf(stderr, __VA_ARGS__);                         \
      fprintf(stderr, "\n");                                \
    }                                                       \
  } while (0)

struct Input {
  int64_t n = 0, M = 0;
  std::vector<double> coef, sg, cw, rec, pk, lm;
  std::vector<int64_t> rows;
};

static bool read_input(const char* path, Input& in) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int64_t hdr[2];
  if (fread(hdr, sizeof(int64_t), 2, f) != 2) { fclose(f); return false; }
  in.n = hdr[0];
  in.M = hdr[1];
  auto rd = [&](std::vector<double>& v, size_t count) { v.resize(count); return count == 0 || fread(v.data(), sizeof(double), count, f) == count; };
  bool ok = rd(in.coef, in.n * 9) && rd(in.sg, in.n * 6) && rd(in.cw, in.n * 4) && rd(in.rec, in.n * 54) && rd(in.pk, in.n * 9) && rd(in.lm, 2);
  in.rows.resize(in.n);
  ok = ok && (in.n == 0 || fread(in.rows.data(), sizeof(int64_t), in.n, f) == (size_t)in.n);
  fclose(f);
  return ok;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

// ---- the law table of dxmat.hip as plan_transfer sees it, and a request with the handle's default options ----------------------
struct LawRow { int law, n_grad, n_isv_fields, isv_dim[DXM_MAX_STATE_FIELDS]; unsigned layouts; };   // layouts: bit per DXM_TANGENT_*
static const LawRow kLawRows[] = {
    {DXM_LAW_ELASTIC_ISO, 6, 0, {0, 0, 0, 0}, 0x3},      // full, sym
    {DXM_LAW_J2_LINEAR, 6, 2, {1, 6, 0, 0}, 0xf},        // all four
    {DXM_LAW_J2_VOCE, 6, 2, {1, 6, 0, 0}, 0xf},
    {DXM_LAW_FEFP_J2_VOCE, 9, 2, {1, 6, 0, 0}, 0x1},     // full only
    {DXM_LAW_FEFP_J2_LINEAR, 9, 2, {1, 6, 0, 0}, 0x1},
    {DXM_LAW_RAMBERG_OSGOOD, 6, 0, {0, 0, 0, 0}, 0xf},   // stateless
};
enum { ELASTIC, J2_LINEAR, J2_VOCE, FEFP_VOCE, FEFP_LINEAR, RAMBERG_OSGOOD };

static TransferRequest request(int law_row, int layout, int64_t n) {
  const LawRow& l = kLawRows[law_row];
  TransferRequest r{};
  r.law = l.law;
  r.n_grad = r.n_flux = l.n_grad;
  r.n_isv_fields = l.n_isv_fields;
  for (int f = 0; f < DXM_MAX_STATE_FIELDS; ++f) r.isv_dim[f] = l.isv_dim[f];
  r.layout = layout;
  r.tangent_size = layout == DXM_TANGENT_SYM ? 21 : layout == DXM_TANGENT_COEF ? 9 : layout == DXM_TANGENT_PACK4 ? 4 : l.n_grad * l.n_grad;
  r.n = n;
  r.flux = r.ct = true;
  r.flux_locked = r.isv_locked = r.ct_locked = true;
  r.packed_transfer = 2;
  r.packed_min_points = 32768;
  r.split_streams = r.pipeline = true;
  r.max_chunks = MAX_CHUNKS;
  return r;
}

// ---- A. the chunk pipeline of run_and_download (dxmat.hip) with the device played by memcpy ---------------------------------
// Per chunk: stage it into its ring slot on the worker threads (`ahead` chunks ahead), wait for the copy, "upload" the slot,
// hand the chunk to the workers with the product's submit_chunk, for the plans of four rebuilt forms.  Returns the rebuilt blocks;
// checks the staged gradient arrived intact.
struct Rebuilt { std::vector<double> ct_coef, ct_pack4, ct_fefp, ct_const, ct_sym; };

static Rebuilt run_pipeline(const Input& in, int threads, int max_chunks, int ahead, HostPool* shared = nullptr) {
  const int64_t n = in.n;
  Rebuilt out;
  out.ct_coef.assign(n * 36, -1.0);
  out.ct_pack4.assign(n * 36, -1.0);
  out.ct_fefp.assign(n * 81, -1.0);
  out.ct_const.assign(n * 36, -1.0);
  out.ct_sym.assign(n * 21, -1.0);
  HostPool* own = shared ? nullptr : new HostPool(threads);
  HostPool& pool = shared ? *shared : *own;
  // a pageable gradient array staged through the ring, the packed forms at any size; the stress landed in the caller's array
  auto plan_of = [&](int law_row, int layout, int packed_transfer) {
    TransferRequest r = request(law_row, layout, n);
    r.staged_grad = true;
    r.packed_transfer = packed_transfer;
    r.packed_min_points = 0;
    r.max_chunks = max_chunks;
    return plan_transfer(r);
  };
  std::vector<double> stress = in.sg;
  auto targets = [&](std::vector<double>& ct, const std::vector<double>& h_coef) {
    return ChunkTargets{stress.data(), ct.data(), h_coef.data(), nullptr, nullptr, nullptr, nullptr, in.lm.data()};
  };
  const TransferPlan plans[4] = {plan_of(J2_LINEAR, DXM_TANGENT_FULL, 1), plan_of(J2_VOCE, DXM_TANGENT_FULL, 2), plan_of(J2_LINEAR, DXM_TANGENT_SYM, 2),
                                 plan_of(FEFP_LINEAR, DXM_TANGENT_FULL, 1)};
  const ChunkTargets tgts[4] = {targets(out.ct_coef, in.coef), targets(out.ct_pack4, in.cw), targets(out.ct_sym, in.cw), targets(out.ct_fefp, in.rec)};
  const TransferPlan constant = plan_of(ELASTIC, DXM_TANGENT_FULL, 2);
  CHECK(plans[0].job == 9 && plans[1].job == 4 && plans[2].job == -4 && plans[3].job == 54 && constant.ct == CtRoute::fill, "pipeline plans");
  const ChunkPlan plan = plans[0].chunks;
  for (const TransferPlan& p : plans)
    CHECK(p.chunks.nchunks == plan.nchunks && p.chunks.csize == plan.csize && p.chunk_jobs, "the four plans cut the batch alike");
  const int ng = 6;
  std::vector<double> ring((size_t)plan.csize * ng * RING, 0.0), d_grad((size_t)n * ng, 0.0);
  const double* host_grad = in.sg.data();   // any (n, 6) array serves as the caller's pageable gradient
  bool slot_busy[RING] = {};
  auto stage = [&](int p) {
    const int64_t cnt = plan.count(p, n);
    if (p >= plan.nchunks || cnt == 0) return;
    CHECK(!slot_busy[ring_slot(p)], "ring slot %d still holds chunk %d when chunk %d is staged", ring_slot(p), p - RING, p);
    slot_busy[ring_slot(p)] = true;
    pool.copy_async(host_grad + plan.offset(p) * ng, ring.data() + (size_t)ring_slot(p) * plan.csize * ng, sizeof(double) * cnt * ng, p);
  };
  if (!shared) pool.submit(in.lm.data(), out.ct_const.data(), n, 0);   // CtRoute::fill, as run_and_download: nothing to wait for
  for (int p = 0; p < ahead; ++p) stage(p);
  for (int c = 0; c < plan.nchunks; ++c) {
    const int64_t off = plan.offset(c), cnt = plan.count(c, n);
    if (cnt == 0) break;
    stage(c + ahead);
    pool.wait_copy(c);
    memcpy(d_grad.data() + off * ng, ring.data() + (size_t)ring_slot(c) * plan.csize * ng, sizeof(double) * cnt * ng);   // the copy kernel
    slot_busy[ring_slot(c)] = false;                                                                                      // ring_done[slot]
    for (int k = 0; k < 4; ++k) submit_chunk(pool, plans[k], tgts[k], c);
  }
  if (shared) {
    pool.submit(in.lm.data(), out.ct_const.data(), n, 0);
  }
  for (int t = 0; t < MAX_CHUNKS; ++t) pool.wait_copy(t);
  pool.wait();
  CHECK(n == 0 || memcmp(d_grad.data(), host_grad, sizeof(double) * n * ng) == 0, "staged gradient differs (max_chunks %d, ahead %d)", max_chunks, ahead);
  delete own;
  return out;
}

static void test_pipeline(const Input& in, FILE* fout) {
  const int64_t n = in.n;
  // serial reference: the same routines on this thread
  Rebuilt ref;
  ref.ct_coef.assign(n * 36, 0.0); ref.ct_pack4.assign(n * 36, 0.0); ref.ct_fefp.assign(n * 81, 0.0); ref.ct_const.assign(n * 36, 0.0);
  expand_coef_tangent(in.coef.data(), ref.ct_coef.data(), n);
  expand_pack4_tangent(in.sg.data(), in.cw.data(), ref.ct_pack4.data(), n);
  expand_fefp_tangent(in.rec.data(), ref.ct_fefp.data(), n);
  fill_const_tangent(in.lm.data(), ref.ct_const.data(), n);
  // the 21-entry form is the upper triangle of the 36-entry one, bit for bit
  ref.ct_sym.assign(n * 21, 0.0);
  expand_pack4_tangent_sym(in.sg.data(), in.cw.data(), ref.ct_sym.data(), n);
  for (int64_t p = 0; p < n; ++p) {
    int t = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j, ++t)
        CHECK(memcmp(&ref.ct_sym[p * 21 + t], &ref.ct_pack4[p * 36 + i * 6 + j], 8) == 0 && memcmp(&ref.ct_pack4[p * 36 + i * 6 + j], &ref.ct_pack4[p * 36 + j * 6 + i], 8) == 0,
              "sym rebuild: entry (%d, %d) of point %" PRId64, i, j, p);
    if (g_failures > 5) break;
  }
  const int chunk_caps[] = {1, 2, 3, 7, 16, 17, 31, 33, 64};
  for (int cap : chunk_caps)
    for (int ahead : {1, 3, RING - 2})
      for (int threads : {1, 5, 16}) {
        if (threads == 16 && cap != 64 && cap != 17) continue;   // keep the sanitizer runs short
        Rebuilt got = run_pipeline(in, threads, cap, ahead);
        CHECK(same_bits(got.ct_coef, ref.ct_coef) && same_bits(got.ct_pack4, ref.ct_pack4) && same_bits(got.ct_fefp, ref.ct_fefp) && same_bits(got.ct_const, ref.ct_const) &&
                  same_bits(got.ct_sym, ref.ct_sym),
              "pipeline result differs from the serial rebuild (max_chunks %d, ahead %d, %d threads)", cap, ahead, threads);
      }
  // rows mode (dxm_integrate_rows): blocks and stress delivered through the index into arrays of M rows
  const int64_t M = in.M;
  std::vector<double> ct_rows(M * 36, 7.0), fx_rows(M * 6, 7.0), ct9_rows(M * 81, 7.0), fx9_rows(M * 9, 7.0), ctc_rows(M * 36, 7.0), fxc_rows(M * 6, 7.0), fld6_rows(M * 6, 7.0), fld1_rows(M, 7.0);
  {
    HostPool pool(16);
    // the plans of the rows forms (a pageable gradient: short chunks on two alternating streams) for J2 with both state fields
    // bound, FeFp and the elastic law; what lands in h_coef / h_flux / h_isv is played by the input arrays
    auto rows_plan = [&](int law_row, unsigned bound) {
      TransferRequest r = request(law_row, DXM_TANGENT_FULL, n);
      r.rows = r.staged_grad = true;
      r.bound_fields = bound;
      return plan_transfer(r);
    };
    const TransferPlan j2 = rows_plan(J2_LINEAR, 0x3), fefp = rows_plan(FEFP_VOCE, 0), cst = rows_plan(ELASTIC, 0);
    CHECK(j2.ct == CtRoute::rows_rebuild && j2.job == 4 && j2.fields == Route::rows && fefp.ct == CtRoute::rows_rebuild && fefp.job == 54 &&
              cst.ct == CtRoute::rows_fill, "rows plans");
    std::vector<double> h_isv(in.cw.begin(), in.cw.begin() + n);   // field-major: p (the first n doubles of cw), then epsp (sg)
    h_isv.insert(h_isv.end(), in.sg.begin(), in.sg.end());
    double* fields[DXM_MAX_STATE_FIELDS] = {fld1_rows.data(), fld6_rows.data(), nullptr, nullptr};
    const int64_t* rw = in.rows.data();
    const ChunkTargets t_j2{fx_rows.data(), ct_rows.data(), in.cw.data(), in.sg.data(), h_isv.data(), fields, rw, in.lm.data()};
    const ChunkTargets t_fefp{fx9_rows.data(), ct9_rows.data(), in.rec.data(), in.pk.data(), nullptr, nullptr, rw, in.lm.data()};
    const ChunkTargets t_cst{fxc_rows.data(), ctc_rows.data(), nullptr, in.sg.data(), nullptr, nullptr, rw, in.lm.data()};
    for (int c = 0; c < j2.chunks.nchunks; ++c) {
      if (j2.chunks.count(c, n) == 0) break;
      submit_chunk(pool, j2, t_j2, c);
      submit_chunk(pool, fefp, t_fefp, c);
      submit_chunk(pool, cst, t_cst, c);
    }
    pool.wait();
  }
  std::vector<char> hit(M, 0);
  for (int64_t p = 0; p < n; ++p) {
    const int64_t r = in.rows[p];
    hit[r] = 1;
    CHECK(memcmp(ct_rows.data() + r * 36, ref.ct_pack4.data() + p * 36, 288) == 0 && memcmp(fx_rows.data() + r * 6, in.sg.data() + p * 6, 48) == 0, "rows mode (pack4): point %" PRId64, p);
    CHECK(memcmp(ct9_rows.data() + r * 81, ref.ct_fefp.data() + p * 81, 648) == 0 && memcmp(fx9_rows.data() + r * 9, in.pk.data() + p * 9, 72) == 0, "rows mode (fefp): point %" PRId64, p);
    CHECK(memcmp(ctc_rows.data() + r * 36, ref.ct_const.data() + p * 36, 288) == 0 && memcmp(fxc_rows.data() + r * 6, in.sg.data() + p * 6, 48) == 0, "rows mode (constant): point %" PRId64, p);
    CHECK(memcmp(fld6_rows.data() + r * 6, in.sg.data() + p * 6, 48) == 0 && fld1_rows[r] == in.cw[p], "rows mode (state fields): point %" PRId64, p);
    if (g_failures > 5) break;
  }
  for (int64_t r = 0; r < M; ++r)
    if (!hit[r]) { CHECK(ct_rows[r * 36] == 7.0 && fx_rows[r * 6] == 7.0 && ct9_rows[r * 81 + 80] == 7.0, "rows mode wrote row %" PRId64 " that no point maps to", r); if (g_failures > 5) break; }
  if (fout) {
    fwrite(ref.ct_coef.data(), sizeof(double), ref.ct_coef.size(), fout);
    fwrite(ref.ct_pack4.data(), sizeof(double), ref.ct_pack4.size(), fout);
    fwrite(ref.ct_fefp.data(), sizeof(double), ref.ct_fefp.size(), fout);
    fwrite(ref.ct_const.data(), sizeof(double), ref.ct_const.size(), fout);
  }
  printf("ok pipeline (n = %" PRId64 ")\n", n);
}

// ---- B. many producers ------------------------------------------------------------------------------------------------------
static void test_many_producers(const Input& in) {
  Rebuilt ref = run_pipeline(in, 4, 16, 3);
  // one pool per producer (HIPMaterial(devices=[...]): one handle, one pool per GPU, side by side)
  {
    std::vector<std::thread> producers;
    std::vector<Rebuilt> got(6);
    for (int t = 0; t < 6; ++t) producers.emplace_back([&, t] { got[t] = run_pipeline(in, 3 + t, 8 + 9 * t, 1 + t % 3); });
    for (auto& th : producers) th.join();
    for (int t = 0; t < 6; ++t)
      CHECK(same_bits(got[t].ct_coef, ref.ct_coef) && same_bits(got[t].ct_pack4, ref.ct_pack4) && same_bits(got[t].ct_fefp, ref.ct_fefp), "producer %d with its own pool", t);
  }
  // several producers on ONE pool, each with its own copy tags (tags are per chunk: disjoint ranges of them here)
  {
    HostPool pool(8);
    const int64_t n = in.n;
    std::vector<std::vector<double>> outs(4, std::vector<double>(n * 36, 0.0));
    std::vector<std::vector<double>> copies(4, std::vector<double>(n * 6, 0.0));
    std::vector<std::thread> producers;
    for (int t = 0; t < 4; ++t)
      producers.emplace_back([&, t] {
        const int64_t per = (n + 7) / 8;
        for (int c = 0; c < 8; ++c) {
          const int64_t off = c * per, cnt = std::max<int64_t>(0, std::min(per, n - off));
          if (cnt == 0) break;
          pool.copy_async(in.sg.data() + off * 6, copies[t].data() + off * 6, sizeof(double) * cnt * 6, t * 16 + c);
          pool.submit(in.cw.data() + off * 4, outs[t].data() + off * 36, cnt, 4, in.sg.data() + off * 6);
          pool.wait_copy(t * 16 + c);
        }
        pool.wait();   // waits for everybody's rebuild jobs: later than needed, never earlier
      });
    for (auto& th : producers) th.join();
    for (int t = 0; t < 4; ++t)
      CHECK(same_bits(outs[t], ref.ct_pack4) && memcmp(copies[t].data(), in.sg.data(), sizeof(double) * n * 6) == 0, "producer %d on the shared pool", t);
  }
  // pools created and destroyed while idle, with work queued, and right after work
  // (the destructor finishes whatever is still queued before it joins: the output array must outlive the pool)
  for (int k = 0; k < 50; ++k) {
    std::vector<double> o(64 * 36);
    HostPool pool(1 + k % 7);
    if (k % 3) pool.submit(in.coef.data(), o.data(), std::min<int64_t>(64, in.n), 9);
    if (k % 3 == 1) pool.wait();
  }
  printf("ok many producers\n");
}

// ---- C. page-locked range table -------------------------------------------------------------------------------------------
static void test_locked_table() {
  LockedTable t;
  std::vector<char> a(4096), b(4096);
  t.note(a.data(), 1000);
  CHECK(t.contains(a.data(), 1000) && t.contains(a.data() + 10, 990) && t.contains(a.data() + 999, 1), "sub-ranges of a noted range");
  CHECK(!t.contains(a.data(), 1001) && !t.contains(a.data() + 999, 2) && !t.contains(a.data() + 1000, 1), "ranges that extend past the noted one");
  CHECK(!t.contains(b.data(), 1) && !t.contains(a.data() - 1, 2), "foreign memory");
  t.note(a.data() + 1000, 1000);   // adjacent: a range that spans both is NOT inside one noted range
  CHECK(t.contains(a.data() + 1000, 1000) && !t.contains(a.data() + 500, 1000), "adjacent ranges are not merged");
  t.forget(a.data());
  CHECK(!t.contains(a.data(), 1) && t.contains(a.data() + 1500, 10), "forget removes exactly one range");
  t.note(a.data(), 50);            // the address comes back with a shorter length
  CHECK(t.contains(a.data(), 50) && !t.contains(a.data(), 51), "re-noted with a shorter length");
  t.forget(a.data());
  t.forget(a.data() + 1000);
  t.forget(b.data());              // never noted: no effect
  CHECK(t.ranges.empty(), "table empty at the end");
  // concurrent note / contains / forget on disjoint and on shared addresses
  std::vector<std::vector<char>> bufs(8, std::vector<char>(1 << 12));
  std::atomic<int> wrong{0};
  std::vector<std::thread> ths;
  for (int k = 0; k < 8; ++k)
    ths.emplace_back([&, k] {
      for (int it = 0; it < 2000; ++it) {
        t.note(bufs[k].data(), 1 << 12);
        if (!t.contains(bufs[k].data() + (it % 4000), 8)) ++wrong;
        (void)t.contains(bufs[(k + 1) % 8].data(), 16);   // somebody else's range: either answer, no race
        t.forget(bufs[k].data());
        if (t.contains(bufs[k].data(), 1)) ++wrong;
      }
    });
  for (auto& th : ths) th.join();
  CHECK(wrong.load() == 0, "%d wrong answers under concurrency", wrong.load());
  printf("ok locked table\n");
}

// ---- D. threaded copies and row moves -------------------------------------------------------------------------------------
static void test_copies() {
  std::mt19937_64 rng(5);
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)7283, (int64_t)300001}) {
    for (int width : {1, 6, 9, 36}) {
      if (n > 100000 && width == 9) continue;
      const int64_t M = 2 * n + 3;
      std::vector<int64_t> rows(n);
      std::vector<int64_t> perm(M);
      for (int64_t i = 0; i < M; ++i) perm[i] = i;
      std::shuffle(perm.begin(), perm.end(), rng);
      for (int64_t i = 0; i < n; ++i) rows[i] = perm[i];
      std::vector<double> src(n * width), dst(M * width, -3.0), ref(M * width, -3.0), back(n * width, 0.0);
      for (auto& v : src) v = (double)(rng() % 100000) / 7.0;
      for (int64_t i = 0; i < n; ++i) memcpy(ref.data() + rows[i] * width, src.data() + i * width, sizeof(double) * width);
      for (int threads : {1, 16, 64, 0}) {
        std::fill(dst.begin(), dst.end(), -3.0);
        move_rows(true, dst.data(), src.data(), rows.data(), n, width, threads);
        CHECK(same_bits(dst, ref), "scatter n=%" PRId64 " width=%d threads=%d", n, width, threads);
        move_rows(false, back.data(), dst.data(), rows.data(), n, width, threads);
        CHECK(same_bits(back, src), "gather n=%" PRId64 " width=%d threads=%d", n, width, threads);
      }
      int64_t lo, hi;
      index_min_max(rows.data(), n, 16, &lo, &hi);
      if (n > 0) {
        CHECK(lo == *std::min_element(rows.begin(), rows.end()) && hi == *std::max_element(rows.begin(), rows.end()), "index_min_max n=%" PRId64, n);
      } else {
        CHECK(lo == INT64_MAX && hi == INT64_MIN, "index_min_max of an empty index");
      }
    }
  }
  for (uint64_t bytes : {(uint64_t)0, (uint64_t)1, (uint64_t)4095, (uint64_t)(4u << 20), (uint64_t)(4u << 20) + 1, (uint64_t)37000001}) {
    std::vector<char> a(bytes + 1, 0), b(bytes + 1, 0x55);
    for (uint64_t i = 0; i < bytes; ++i) a[i] = (char)(i * 131 + 7);
    for (int threads : {0, 1, 3, 16, 200}) {
      std::fill(b.begin(), b.end(), 0x55);
      host_copy(b.data(), a.data(), bytes, threads);
      CHECK((bytes == 0 || memcmp(a.data(), b.data(), bytes) == 0) && b[bytes] == 0x55, "host_copy of %" PRIu64 " bytes on %d threads", bytes, threads);
    }
  }
  printf("ok copies and row moves\n");
}

// ---- E. chunk planner, ring slots, status-record capacity -----------------------------------------------------------------
static void test_planner() {
  std::vector<int64_t> sizes = {0, 1, 63, 64, 65, 255, 256, 257, 32767, 32768, 32769, 65535, 65536, 131071, 131072, 131073, 1000003, 2097151, 2097152, 2097153,
                                9999999, 10000000, 10000001, 12500000, 19999999, 20000000, 100000000};
  std::mt19937_64 rng(11);
  for (int k = 0; k < 400; ++k) sizes.push_back((int64_t)(rng() % 20000001));
  int64_t checked = 0;
  for (int64_t n : sizes)
    for (int cap = 1; cap <= MAX_CHUNKS; ++cap)
      for (int flags = 0; flags < 8; ++flags) {
        const bool packed = flags & 1, staged = flags & 2, pipeline = flags & 4;
        const ChunkPlan p = plan_chunks(n, packed, staged, cap, pipeline);
        ++checked;
        CHECK(p.nchunks >= 1 && p.nchunks <= cap && p.nchunks <= MAX_CHUNKS && (pipeline || p.nchunks == 1), "nchunks %d (n %" PRId64 ", cap %d, flags %d)", p.nchunks, n, cap, flags);
        CHECK(p.csize % 256 == 0 && (n == 0 || p.csize > 0), "chunk size %" PRId64 " not a multiple of 256", p.csize);
        int64_t covered = 0;
        int64_t records[4] = {0, 0, 0, 0};
        const int bpc[4] = {1, 5, 32, 256};
        for (int c = 0; c < p.nchunks; ++c) {
          const int64_t cnt = p.count(c, n);
          CHECK(cnt == 0 || p.offset(c) == covered, "chunk %d starts at %" PRId64 ", expected %" PRId64, c, p.offset(c), covered);
          CHECK(p.offset(c) % 256 == 0, "chunk offset not a multiple of 256");
          covered += cnt;
          if (cnt > 0)
            for (int b = 0; b < 4; ++b) records[b] += launch_grid(cnt, 256, bpc[b]);
        }
        CHECK(covered == n, "chunks cover %" PRId64 " of %" PRId64 " points", covered, n);
        CHECK(p.issued(n) <= p.nchunks && (n == 0 || p.count(p.issued(n) - 1, n) > 0) && p.count(p.issued(n), n) == 0, "issued() disagrees with count()");
        for (int b = 0; b < 4; ++b)
          CHECK(records[b] <= stats_capacity(256, n), "status records %" PRId64 " exceed the capacity %d (n %" PRId64 ", cap %d, flags %d, %d blocks/CU)", records[b], stats_capacity(256, n), n, cap, flags, bpc[b]);
        if (g_failures > 20) return;
      }
  // a slot is reused by chunk c + RING and by no chunk in between; `ahead` <= RING - 2 chunks in flight never collide
  for (int c = 0; c < 4 * RING; ++c)
    for (int d = 1; d < RING; ++d) CHECK(ring_slot(c) != ring_slot(c + d), "ring slot collision between chunks %d and %d", c, c + d);
  CHECK(ring_slot(5) == ring_slot(5 + RING), "ring period");
  CHECK(stats_capacity(256, 0) == 256 * 256 && stats_capacity(304, (int64_t)1 << 40) == INT32_MAX, "capacity limits");
  printf("ok planner (%" PRId64 " plans)\n", checked);
}

// ---- F. upload-route state machine ------------------------------------------------------------------------------------------
static void test_chooser() {
  {   // option 1: call 1 not judged, calls 2-5 alternate, the faster way is kept, the other is probed every 32nd call
    UploadChooser u;
    std::vector<int> ways;
    auto call = [&](double ms1, double ms2) {
      int w = u.choose();
      if (w == 1) u.registered(1.0, (size_t)480e6);
      ways.push_back(w);
      u.record(w, w == 1 ? ms1 : ms2);
      return w;
    };
    for (int k = 0; k < 5; ++k) call(24.0, 31.0);
    CHECK((ways == std::vector<int>{1, 1, 2, 1, 2}), "calibration sequence");
    CHECK(u.pref == 1 && u.ms[1] == 24.0 && u.ms[2] == 31.0, "page-locking kept (24 vs 31 ms)");
    int probes = 0;
    for (int k = 0; k < 64; ++k) probes += call(24.0, 31.0) == 2;
    CHECK(probes == 2 && u.pref == 1, "two probes of the other way in 64 calls, preference unchanged");
    for (int k = 0; k < 40; ++k) call(40.0, 30.0);   // the host changed: staging is now faster; the next probe finds out
    CHECK(u.pref == 2, "switched to staging after a probe (pref %d)", u.pref);
  }
  {   // a tie within 5 % goes to page-locking
    UploadChooser u;
    for (int k = 0; k < 5; ++k) { int w = u.choose(); u.record(w, w == 1 ? 25.0 : 24.0); }
    CHECK(u.pref == 1, "tie within 5 %% keeps page-locking");
    UploadChooser v;
    for (int k = 0; k < 5; ++k) { int w = v.choose(); v.record(w, w == 1 ? 25.0 : 23.0); }
    CHECK(v.pref == 2, "8 %% faster staging wins");
  }
  {   // expensive registrations (small pages): three in a row after the first send 20 calls through the ring
    UploadChooser u;
    u.set_option(2);
    int staged = 0, total = 0;
    for (int k = 0; k < 30; ++k) {
      int w = u.choose();
      ++total;
      if (w == 1) u.registered(12.0, (size_t)480e6); else ++staged;   // 24 ms/GB
      u.record(w, 30.0);
    }
    // call 1 registers and is not judged, calls 2-4 are slow -> calls 5-24 staged, calls 25-27 slow again -> 28-30 staged
    CHECK(staged == 23 && total == 30, "23 of 30 calls staged around two runs of three slow registrations (got %d)", staged);
    UploadChooser r;
    r.set_option(2);
    CHECK(r.choose() == 1, "option 2 page-locks");
    r.refused();
    for (int k = 0; k < 20; ++k) CHECK(r.choose() == 2, "refusal: staged for 20 calls");
    CHECK(r.choose() == 1, "then one more try");
  }
  {   // option 0 never registers; set_option resets the calibration
    UploadChooser u;
    u.set_option(0);
    for (int k = 0; k < 10; ++k) { CHECK(u.choose() == 0, "option 0"); u.record(0, 20.0); }
    CHECK(u.calls == 0, "option 0 does not count calls");
    u.set_option(1);
    for (int k = 0; k < 7; ++k) { int w = u.choose(); u.record(w, 20.0); }
    u.set_option(1);
    CHECK(u.calls == 0 && u.pref == 1 && u.ms[1] == 0.0 && u.ms[2] == 0.0 && !u.probing, "set_option resets the calibration");
  }
  printf("ok upload chooser\n");
}

// ---- G. transfer plans of the host-buffer form ------------------------------------------------------------------------------------
// What run_and_download does with a plan, checked against the request it came from.
static void check_plan(const TransferPlan& p) {
  const TransferRequest& r = p.req;
  int total = 0;
  for (int f = 0; f < r.n_isv_fields; ++f) total += r.isv_dim[f];
  const bool rows_job = p.ct == CtRoute::rows_move || p.ct == CtRoute::rows_rebuild || p.ct == CtRoute::rows_fill;   // stress along
  // every requested destination is written by exactly one route, the others by none
  const int flux_writers = (p.flux == Route::dma) + (p.flux == Route::staged) + (p.flux == Route::rows && rows_job);
  CHECK(flux_writers == (r.flux ? 1 : 0) && (p.flux != Route::rows || rows_job), "flux written %d times", flux_writers);
  CHECK((p.ct != CtRoute::none) == r.ct, "tangent route %d, requested %d", (int)p.ct, (int)r.ct);
  CHECK((p.isv != Route::none) == (r.isv_aos && total > 0) && p.isv != Route::rows, "isv route %d", (int)p.isv);
  CHECK((p.fields != Route::none) == (r.bound_fields != 0) && p.fields != Route::staged, "field route %d", (int)p.fields);
  // the rows forms never DMA into caller memory, the others never scatter
  if (r.rows)
    CHECK(p.flux == Route::rows && rows_job && p.isv == Route::none && p.fields != Route::dma, "rows form with a DMA into the caller's memory");
  else
    CHECK(!rows_job && p.flux != Route::rows && p.fields != Route::rows, "rows route without rows");
  // no two layouts share one device scratch: interleaved isv rows and field-major fields never both in d_isv
  CHECK(p.fields_own_scratch == (p.isv != Route::none && p.fields != Route::none), "field scratch");
  // widths: d_ct holds n_flux * n_grad doubles per point, h_coef `land`
  CHECK(p.nt >= 1 && p.nt <= r.n_flux * r.n_grad, "nt %d", p.nt);
  CHECK(!p.need_h_coef || (p.np >= 1 && p.np <= p.land), "np %d > land %d", p.np, p.land);
  CHECK(!p.ct_lands() || p.nt == p.np, "what the kernel writes (%d) is not what lands (%d)", p.nt, p.np);
  CHECK(p.need_h_coef == p.ct_lands(), "h_coef needed %d, tangent lands %d", (int)p.need_h_coef, (int)p.ct_lands());
  if (p.ct == CtRoute::none || p.ct == CtRoute::fill || p.ct == CtRoute::dma || p.ct == CtRoute::staged || p.ct == CtRoute::rows_fill)
    CHECK(p.tl == r.layout && p.nt == r.tangent_size, "an unpacked tangent launched as layout %d", p.tl);
  // pack4 and sym rebuilds read the stress: it lands in page-locked memory or h_flux
  if ((p.ct == CtRoute::rebuild || p.ct == CtRoute::rows_rebuild) && (p.job == 4 || p.job == -4))
    CHECK(p.tl == DXM_TANGENT_PACK4 && (p.flux == Route::dma || p.flux == Route::rows), "a stress-based rebuild without the stress landed");
  // chunks
  const int cap = std::min(r.max_chunks, MAX_CHUNKS);
  CHECK(p.split_cap >= 1 && p.split_cap <= 24, "split cap %d", p.split_cap);
  CHECK(p.chunks.nchunks >= 1 && p.chunks.nchunks <= cap && (r.pipeline || p.chunks.nchunks == 1), "%d chunks", p.chunks.nchunks);
  if (p.split) CHECK(p.chunks.nchunks > 1 && p.chunks.nchunks <= std::min(p.split_cap, r.max_chunks), "split into %d chunks", p.chunks.nchunks);
  CHECK(!p.split || (!r.staged_grad && !r.fused && r.split_streams && r.pipeline), "split with staged / fused / option off");
  // the pool whenever a worker job or the staging ring is needed
  const bool worker_jobs = p.ct == CtRoute::fill || p.chunk_jobs || p.fields == Route::rows;
  CHECK(p.need_pool == (p.packed || r.staged_grad) && (!(worker_jobs || r.staged_grad) || p.need_pool), "pool");
  CHECK(p.chunk_jobs == (p.ct == CtRoute::rebuild || rows_job), "chunk jobs %d for tangent route %d", (int)p.chunk_jobs, (int)p.ct);
  CHECK(p.need_h_flux == (p.flux == Route::rows) && p.need_h_isv == (p.fields == Route::rows), "landing areas");
}

static void test_transfer_plans() {
  // the whole valid product: law x layout, rows form, destinations, bound fields, gradient route, options, locked flags, sizes, caps
  const int64_t min_points = 32768;
  const int64_t sizes[] = {1, 255, min_points - 1, min_points, 300000, 1000003, 10000000, 100000000};
  const int caps[] = {1, 7, MAX_CHUNKS};
  int64_t count = 0;
  for (int law = 0; law < (int)(sizeof(kLawRows) / sizeof(kLawRows[0])); ++law)
    for (int layout = 0; layout < 4; ++layout) {
      if (!(kLawRows[law].layouts >> layout & 1)) continue;
      for (int rows = 0; rows < 2; ++rows)
        for (int present = 0; present < 8; ++present) {   // flux, isv_aos, ct
          const bool flux = present & 1, isv = present & 2, ct = present & 4;
          if (rows && (!flux || !ct || isv)) continue;   // the rows forms: flux and tangent, never isv_aos
          for (unsigned bound = 0; bound < (1u << kLawRows[law].n_isv_fields); ++bound)
            for (int grad = 0; grad < 3; ++grad)            // page-locked (DMA), staged, fused
              for (int pt = 0; pt < 3; ++pt)
                for (int opts = 0; opts < 4; ++opts)        // split_streams, pipeline
                  for (int locked = 0; locked < 8; ++locked)
                    for (int64_t n : sizes)
                      for (int cap : caps) {
                        TransferRequest r = request(law, layout, n);
                        r.rows = rows;
                        r.flux = flux;
                        r.isv_aos = isv;
                        r.ct = ct;
                        r.bound_fields = bound;
                        r.staged_grad = grad == 1;
                        r.fused = grad == 2;
                        r.packed_transfer = pt;
                        r.split_streams = opts & 1;
                        r.pipeline = opts & 2;
                        r.flux_locked = locked & 1;
                        r.isv_locked = locked & 2;
                        r.ct_locked = locked & 4;
                        r.max_chunks = cap;
                        check_plan(plan_transfer(r));
                        ++count;
                        if (g_failures > 20) return;
                      }
        }
    }
  // the routes the documentation promises
  int pinned = 0;
  auto pin = [&](int law, int layout, int64_t n, auto edit, auto expect, const char* what) {
    TransferRequest r = request(law, layout, n);
    edit(r);
    const TransferPlan p = plan_transfer(r);
    check_plan(p);
    CHECK(expect(p), "pinned case: %s", what);
    ++pinned;
  };
  auto none = [](TransferRequest&) {};
  pin(J2_LINEAR, DXM_TANGENT_FULL, 1000000, none, [](const TransferPlan& p) {
    return p.ct == CtRoute::rebuild && p.tl == DXM_TANGENT_PACK4 && p.np == 4 && p.nt == 4 && p.job == 4 && p.nfull == 36 && p.flux == Route::dma; },
      "J2, full layout, locked flux: pack4, 4 doubles landed, job 4");
  pin(J2_VOCE, DXM_TANGENT_SYM, 1000000, none, [](const TransferPlan& p) {
    return p.ct == CtRoute::rebuild && p.tl == DXM_TANGENT_PACK4 && p.np == 4 && p.nfull == 21 && p.job == -4; }, "sym: 4 landed, 21 rebuilt, job -4");
  pin(FEFP_VOCE, DXM_TANGENT_FULL, 1000000, none, [](const TransferPlan& p) {
    return p.ct == CtRoute::rebuild && p.tl == DXM_TANGENT_COEF && p.np == 54 && p.job == 54 && p.nfull == 81 && p.land == 54; }, "FeFp: 54 building blocks");
  pin(ELASTIC, DXM_TANGENT_FULL, 1000000, none, [](const TransferPlan& p) {
    return p.ct == CtRoute::fill && !p.need_h_coef && !p.chunk_jobs && p.tl == DXM_TANGENT_FULL; }, "elastic full: constant fill, nothing downloaded");
  pin(J2_LINEAR, DXM_TANGENT_FULL, 32767, none, [](const TransferPlan& p) {
    return p.ct == CtRoute::dma && p.nt == 36 && p.tl == DXM_TANGENT_FULL && !p.need_pool; }, "below packed_min_points: DMA of the full block");
  pin(J2_LINEAR, DXM_TANGENT_SYM, 1000000, [](TransferRequest& r) { r.packed_transfer = 0; }, [](const TransferPlan& p) {
    return p.ct == CtRoute::dma && p.nt == 21 && p.tl == DXM_TANGENT_SYM; }, "packed_transfer 0: DMA of the handle's layout");
  pin(J2_LINEAR, DXM_TANGENT_FULL, 1000000, [](TransferRequest& r) { r.packed_transfer = 1; }, [](const TransferPlan& p) {
    return p.ct == CtRoute::rebuild && p.tl == DXM_TANGENT_COEF && p.np == 9 && p.job == 9; }, "packed_transfer 1: the nine coefficients");
  pin(J2_LINEAR, DXM_TANGENT_FULL, 1000000, [](TransferRequest& r) { r.flux_locked = false; }, [](const TransferPlan& p) {
    return p.ct == CtRoute::rebuild && p.np == 9 && p.flux == Route::staged; }, "pageable flux: the nine coefficients, stress staged");
  pin(J2_LINEAR, DXM_TANGENT_SYM, 1000000, [](TransferRequest& r) { r.rows = true; }, [](const TransferPlan& p) {
    return p.ct == CtRoute::rows_move && p.np == 21 && p.land == 21 && p.tl == DXM_TANGENT_SYM; }, "rows + sym: rows move of 21");
  pin(J2_LINEAR, DXM_TANGENT_FULL, 1000000, [](TransferRequest& r) { r.rows = true; r.bound_fields = 3; }, [](const TransferPlan& p) {
    return p.ct == CtRoute::rows_rebuild && p.job == 4 && p.flux == Route::rows && p.fields == Route::rows && p.need_h_isv; }, "rows + full: pack4 rebuilt into the rows");
  pin(ELASTIC, DXM_TANGENT_FULL, 1000000, [](TransferRequest& r) { r.rows = true; }, [](const TransferPlan& p) {
    return p.ct == CtRoute::rows_fill && !p.need_h_coef && p.chunk_jobs; }, "rows + elastic: constant filled into the rows");
  pin(J2_LINEAR, DXM_TANGENT_FULL, 10000000, [](TransferRequest& r) { r.staged_grad = true; r.packed_transfer = 0; }, [](const TransferPlan& p) {
    return !p.split && p.ct == CtRoute::dma && p.chunks.nchunks == 32; }, "staged gradient, full layout, packed_transfer 0: two alternating streams, 32 chunks");
  pin(J2_LINEAR, DXM_TANGENT_FULL, 300000, none, [](const TransferPlan& p) { return p.split && p.split_cap == 3 && p.chunks.nchunks == 3; },
      "3e5 points: the split cap truncates to 3");
  pin(J2_LINEAR, DXM_TANGENT_FULL, 10000000, none, [](const TransferPlan& p) { return p.split && p.chunks.nchunks == 22; }, "1e7 points: 22 chunks split");
  pin(J2_VOCE, DXM_TANGENT_FULL, 1000000, [](TransferRequest& r) { r.isv_aos = true; r.bound_fields = 2; }, [](const TransferPlan& p) {
    return p.isv == Route::dma && p.fields == Route::dma && p.fields_own_scratch; }, "isv_aos and bound fields: their own scratch");
  printf("ok transfer plans (%" PRId64 " plans, %d pinned cases)\n", count, pinned);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s input.bin [output.bin]\n", argv[0]); return 2; }
  Input in;
  if (!read_input(argv[1], in)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  FILE* fout = argc > 2 ? fopen(argv[2], "wb") : nullptr;
  test_pipeline(in, fout);
  if (fout) fclose(fout);
  test_many_producers(in);
  test_locked_table();
  test_copies();
  test_planner();
  test_chooser();
  test_transfer_plans();
  // ragged and empty batches through the same pipeline
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)257}) {
    Input small = in;
    small.n = std::min(n, in.n);
    small.coef.resize(small.n * 9); small.sg.resize(small.n * 6); small.cw.resize(small.n * 4); small.rec.resize(small.n * 54); small.pk.resize(small.n * 9); small.rows.resize(small.n);
    test_pipeline(small, nullptr);
  }
  if (g_failures) { fprintf(stderr, "%d check(s) failed\n", g_failures); return 1; }
  printf("all ok\n");
  return 0;
}
