// The launch-choice rule of the clean-tile stamps (dolfinx_materials_amd/csrc/host_side.hpp: choose_state_launch, covers_whole_tiles,
// next_clean_stamp), enumerated over every combination of its inputs.  A stand-alone program: tests/test_clean_tiles_host.py builds
// it with -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../dolfinx_materials_amd/csrc/host_side.hpp"

using dxm_host::StateLaunch;
using dxm_host::StateLaunchFlags;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
  } while (0)

int main() {
  int n_clean = 0, n_plain = 0, n_bump = 0;
  for (unsigned bits = 0; bits < (1u << 9); ++bits) {
    StateLaunchFlags f{};
    f.has_stamps = bits & 1u;
    f.option = bits & 2u;
    f.fields = bits & 4u;
    f.frame = bits & 8u;
    f.fused = bits & 16u;
    f.whole_tiles = bits & 32u;
    f.capturing = bits & 64u;
    f.exposed = bits & 128u;
    f.stamps_stale = bits & 256u;
    const StateLaunch how = dxm_host::choose_state_launch(f);
    n_clean += how == StateLaunch::clean;
    n_plain += how == StateLaunch::plain;
    n_bump += how == StateLaunch::plain_bump;
    // never the eliding kernel where a write could go unseen, or where that kernel does not exist
    if (f.capturing || f.exposed || f.fields || f.frame || f.fused || !f.whole_tiles || !f.option || !f.has_stamps || f.stamps_stale)
      CHECK(how != StateLaunch::clean);
    else
      CHECK(how == StateLaunch::clean);
    // every plain launch of a handle that has stamps moves the stamp on; a handle without stamps has nothing to move
    if (f.has_stamps) CHECK(how != StateLaunch::plain);
    else CHECK(how == StateLaunch::plain);
  }
  CHECK(n_clean == 1 && n_plain == 256 && n_bump == 255);

  // whole tiles of the handle: the chunk plan's multiples of 256 with the ragged end of the handle are, a ragged range inside is not
  CHECK(dxm_host::covers_whole_tiles(0, 401, 401));
  CHECK(dxm_host::covers_whole_tiles(0, 1, 1));
  CHECK(dxm_host::covers_whole_tiles(256, 145, 401));
  CHECK(dxm_host::covers_whole_tiles(64, 128, 401));
  CHECK(!dxm_host::covers_whole_tiles(0, 100, 401));
  CHECK(!dxm_host::covers_whole_tiles(32, 369, 401));
  CHECK(!dxm_host::covers_whole_tiles(1, 64, 401));
  for (int64_t n : {1, 63, 64, 65, 401, 131153, 10000000}) {
    const dxm_host::ChunkPlan p = dxm_host::plan_chunks(n, true, false, dxm_host::MAX_CHUNKS, true);
    for (int c = 0; c < p.issued(n); ++c) CHECK(dxm_host::covers_whole_tiles(p.offset(c), p.count(c, n), n));
  }

  // the stamp counter: never 0, wraps once in 2^32 - 1 steps and says so
  bool wrapped = true;
  CHECK(dxm_host::next_clean_stamp(1u, &wrapped) == 2u && !wrapped);
  CHECK(dxm_host::next_clean_stamp(0xfffffffeu, &wrapped) == 0xffffffffu && !wrapped);
  CHECK(dxm_host::next_clean_stamp(0xffffffffu, &wrapped) == 1u && wrapped);
  {
    std::vector<uint32_t> seen;
    uint32_t s = 0xfffffffcu;
    for (int k = 0; k < 8; ++k) { s = dxm_host::next_clean_stamp(s, &wrapped); seen.push_back(s); CHECK(s != 0u); }
    CHECK(seen[2] == 0xffffffffu && seen[3] == 1u && seen[7] == 5u);
  }

  if (failures == 0) std::printf("all ok: %d clean, %d plain, %d plain-and-bump\n", n_clean, n_plain, n_bump);
  return failures == 0 ? 0 : 1;
}
