// Stand-alone harness (its own main, built with -fsanitize=address,undefined by tests/test_log_strain_plane_cpu.py) of the
// transfer-plan branch of law 42 in csrc/host_side.hpp::plan_transfer: the 25 entries of its 5 x 5 tangent cross as they are, in the
// full and the rows forms, no rebuild or fill job is planned, and the plan of every request equals, field by field, that of law 19 and
// that of law 38 handed the same request (same sizes: the plain-block branch, whatever the widths).  Exit status 1 on a broken
// statement.  (Every other law's plans are pinned by the digest of tests/plane_stress_j2_plan_harness.cpp, which does not name this id.)
#include <cstdint>
#include <cstdio>

#include "../dolfinx_materials_amd/csrc/host_side.hpp"

using namespace dxm_host;

static int g_bad = 0;
#define CHECK(cond, what) do { if (!(cond)) { fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); ++g_bad; } } while (0)

static bool same_plan(const TransferPlan& p, const TransferPlan& q, int64_t n) {
  return p.packed == q.packed && p.tl == q.tl && p.nt == q.nt && p.np == q.np && p.land == q.land && p.nfull == q.nfull && p.job == q.job &&
         p.ct == q.ct && p.flux == q.flux && p.isv == q.isv && p.fields == q.fields && p.fields_own_scratch == q.fields_own_scratch &&
         p.chunk_jobs == q.chunk_jobs && p.need_h_coef == q.need_h_coef && p.need_h_flux == q.need_h_flux && p.need_h_isv == q.need_h_isv &&
         p.need_pool == q.need_pool && p.short_chunks == q.short_chunks && p.split_cap == q.split_cap && p.split == q.split &&
         p.chunks.nchunks == q.chunks.nchunks && p.chunks.csize == q.chunks.csize && p.chunks.issued(n) == q.chunks.issued(n);
}

int main() {
  const int64_t sizes[] = {0, 1, 255, 32768, 100003, 264600, 1000000, 10000000};
  long long plans = 0;
  for (int64_t n : sizes)
    for (int bits = 0; bits < 1 << 9; ++bits)
      for (int packed = 0; packed < 3; ++packed) {
        TransferRequest r{};
        r.law = DXM_LAW_LOG_STRAIN_PE; r.n_grad = 5; r.n_flux = 5;
        r.n_isv_fields = 2; r.isv_dim[0] = 4; r.isv_dim[1] = 1;          // ElasticStrain [xx, yy, zz, sqrt(2) xy], EquivalentPlasticStrain
        r.layout = DXM_TANGENT_FULL; r.tangent_size = 25; r.n = n;       // dxm_set_tangent_layout refuses the others
        r.flux = bits & 1; r.isv_aos = bits >> 1 & 1; r.ct = bits >> 2 & 1; r.rows = bits >> 3 & 1; r.staged_grad = bits >> 4 & 1;
        r.fused = bits >> 5 & 1; r.flux_locked = bits >> 6 & 1; r.ct_locked = bits >> 6 & 1; r.isv_locked = bits >> 6 & 1;
        r.split_streams = bits >> 7 & 1; r.pipeline = bits >> 8 & 1;
        if (r.rows && !(r.flux && r.ct)) continue;   // the rows forms need both arrays
        if (r.fused) continue;                       // the displacement forms are refused for this law
        r.packed_transfer = packed; r.packed_min_points = 32768; r.max_chunks = MAX_CHUNKS;
        const TransferPlan p = plan_transfer(r);
        ++plans;
        CHECK(p.tl == DXM_TANGENT_FULL && p.nt == 25 && p.nfull == 25, "the launch writes the 5 x 5 block, 25 numbers per point");
        if (!r.ct) CHECK(p.ct == CtRoute::none, "no tangent asked, none moved");
        else if (r.rows) {
          CHECK(p.ct == CtRoute::rows_move && p.np == 25 && p.land >= 25 && p.need_h_coef && p.need_pool && p.chunk_jobs, "rows form: the 25 entries land and are moved to their rows");
          CHECK(p.flux == Route::rows && p.need_h_flux, "rows form: the flux lands and is moved too");
        } else {
          CHECK(!p.packed && (p.ct == (r.ct_locked ? CtRoute::dma : CtRoute::staged)), "full form: downloaded as it is, whatever option packed_transfer says");
          CHECK(!p.need_h_coef, "full form: no record lands");
        }
        CHECK(p.ct != CtRoute::rebuild && p.ct != CtRoute::rows_rebuild && p.ct != CtRoute::fill && p.ct != CtRoute::rows_fill, "nothing is rebuilt or filled");
        CHECK(p.chunks.nchunks >= 1 && p.chunks.csize % 256 == 0 && p.chunks.offset(p.chunks.nchunks) >= r.n, "the chunks cover the batch");
        CHECK(p.fields == Route::none, "nothing bound, nothing delivered");
        if (n == 264600 && r.ct && !r.rows && r.pipeline) CHECK(p.chunks.nchunks >= 2, "264 600 points cross in more than one chunk");
        TransferRequest r19 = r, r38 = r;
        r19.law = DXM_LAW_LOG_STRAIN_J2;
        r38.law = DXM_LAW_OGDEN_PE;
        CHECK(same_plan(p, plan_transfer(r19), r.n), "the plan is that of law 19 for the same request");
        CHECK(same_plan(p, plan_transfer(r38), r.n), "the plan is that of law 38 for the same request");
      }
  printf("checked %lld plans, %d broken statements\n", plans, g_bad);
  return g_bad ? 1 : 0;
}
