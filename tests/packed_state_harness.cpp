// The rule that decides when a J2 launch builds or reads the packed copy of s0 (dolfinx_materials_amd/csrc/host_side.hpp:
// choose_state_launch with its pack_* inputs, pack_candidate, PackEpoch), enumerated over every combination of its flags and the
// launch counts 0-3 of an s0 epoch, and over every sequence of six events on a handle.  A stand-alone program:
// tests/test_packed_state_host.py builds it with -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>

#include "../dolfinx_materials_amd/csrc/host_side.hpp"

using dxm_host::PackEpoch;
using dxm_host::StateLaunch;
using dxm_host::StateLaunchFlags;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
  } while (0)

static StateLaunchFlags old_flags(unsigned bits) {
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
  return f;
}

// a launch that today's rule gives the clean kernel, with everything the copy asks for
static StateLaunchFlags eligible() {
  StateLaunchFlags f = old_flags(1u | 2u | 32u);
  f.pack_option = true;
  f.full_range = true;
  f.ordered = true;
  return f;
}

int main() {
  // ---- 1. every combination of the flags, launch counts 0-3 ---------------------------------------------------------------
  long n_build = 0, n_use = 0, n_total = 0;
  for (unsigned bits = 0; bits < (1u << 9); ++bits)
    for (unsigned nb = 0; nb < (1u << 5); ++nb)
      for (int launches = 0; launches <= 3; ++launches) {
        const StateLaunch today = dxm_host::choose_state_launch(old_flags(bits));   // the rule without the copy
        StateLaunchFlags f = old_flags(bits);
        f.pack_option = nb & 1u;
        f.full_range = nb & 2u;
        f.chunk_of_host_call = nb & 4u;
        f.built = nb & 8u;
        f.ordered = nb & 16u;
        f.epoch_launches = launches;
        const StateLaunch how = dxm_host::choose_state_launch(f);
        ++n_total;
        n_build += how == StateLaunch::clean_build;
        n_use += how == StateLaunch::clean_use;
        const bool packed = how == StateLaunch::clean_build || how == StateLaunch::clean_use;
        // build and use only where today's rule chooses the clean kernel; everything else is today's answer
        if (today != StateLaunch::clean) CHECK(how == today);
        else CHECK(how == StateLaunch::clean || packed);
        // every condition that keeps a launch off the copy
        if (!f.pack_option || !f.full_range || f.chunk_of_host_call || f.fields || f.frame || f.fused || !f.whole_tiles || f.capturing ||
            f.exposed || !f.option || !f.has_stamps || f.stamps_stale)
          CHECK(!packed);
        // use only behind a build of this epoch, and ordered behind it; build only as the second or a later launch, once
        if (how == StateLaunch::clean_use) CHECK(f.built && f.ordered);
        if (how == StateLaunch::clean_build) CHECK(!f.built && f.epoch_launches >= 1);
        if (f.epoch_launches == 0 && !f.built) CHECK(!packed);
        // ... and where all of that holds, the copy IS used
        if (today == StateLaunch::clean && f.pack_option && f.full_range && !f.chunk_of_host_call) {
          if (f.built) CHECK(how == (f.ordered ? StateLaunch::clean_use : StateLaunch::clean));
          else CHECK(how == (f.epoch_launches >= 1 ? StateLaunch::clean_build : StateLaunch::clean));
        }
        CHECK(dxm_host::pack_candidate(f, how) == (today == StateLaunch::clean && f.pack_option && f.full_range && !f.chunk_of_host_call));
      }
  CHECK(n_total == 512 * 32 * 4);
  // one combination of the nine old flags; pack_option, full_range, no chunk; build: not built, either `ordered`, counts 1-3;
  // use: built and ordered, any count
  CHECK(n_build == 2 * 3 && n_use == 4);

  // ---- 2. the sequence of one epoch: plain, build, use, use -------------------------------------------------------------------
  {
    PackEpoch e;
    const StateLaunch want[4] = {StateLaunch::clean, StateLaunch::clean_build, StateLaunch::clean_use, StateLaunch::clean_use};
    for (int k = 0; k < 4; ++k) {
      StateLaunchFlags f = eligible();
      f.epoch_launches = e.launches;
      f.built = e.built;
      CHECK(f.epoch_launches == (k < 3 ? k : 3));
      const StateLaunch how = dxm_host::choose_state_launch(f);
      CHECK(how == want[k]);
      e.note(f, how);
    }
    e.move();
    CHECK(e.launches == 0 && !e.built);
  }

  // ---- 3. every sequence of six events ------------------------------------------------------------------------------------------
  // 0 an eligible launch; 1 a chunk of a host-buffer call (clean kernel, not a candidate); 2 a launch with parameter fields bound
  // (plain kernel, the stamp moves); 3 an event that may change s0 (advance, dxm_set_state, ...: PackEpoch::move); 4 an eligible
  // launch that cannot be ordered behind the build.  The model: has a build been issued since s0 last may have changed?
  long n_seq = 0, n_use_seq = 0;
  for (int code = 0; code < 5 * 5 * 5 * 5 * 5 * 5; ++code) {
    PackEpoch e;
    bool model_built = false;
    int model_launches = 0;
    int c = code;
    for (int step = 0; step < 6; ++step, c /= 5) {
      const int ev = c % 5;
      if (ev == 3) {
        e.move();
        model_built = false;
        model_launches = 0;
        CHECK(e.launches == 0 && !e.built);
        continue;
      }
      StateLaunchFlags f = eligible();
      if (ev == 1) f.chunk_of_host_call = true;
      if (ev == 2) f.fields = true;
      if (ev == 4) f.ordered = false;
      f.epoch_launches = e.launches;
      f.built = e.built;
      const StateLaunch how = dxm_host::choose_state_launch(f);
      if (how == StateLaunch::clean_use) { CHECK(model_built); ++n_use_seq; }
      if (how == StateLaunch::clean_build) { CHECK(!model_built && model_launches >= 1); model_built = true; }
      if (ev == 1) CHECK(how == StateLaunch::clean);
      if (ev == 2) CHECK(how == StateLaunch::plain_bump);
      if (ev == 0) CHECK(how == (model_built && !(how == StateLaunch::clean_build) ? StateLaunch::clean_use
                                 : model_launches >= 1 ? StateLaunch::clean_build : StateLaunch::clean));
      e.note(f, how);
      if (ev == 2) { model_built = false; model_launches = 0; CHECK(e.launches == 0 && !e.built); }
      else if (ev != 1) ++model_launches;
      CHECK(e.built == model_built && e.launches == (model_launches < 3 ? model_launches : 3));
    }
    ++n_seq;
  }
  CHECK(n_seq == 15625 && n_use_seq > 0);

  if (failures == 0) std::printf("all ok: %ld combinations, %ld build, %ld use; %ld sequences, %ld use launches\n", n_total, n_build, n_use, n_seq, n_use_seq);
  return failures == 0 ? 0 : 1;
}
