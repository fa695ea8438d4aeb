// Host-only check of ck_first_tables (povar_amd/csrc/ck_layout.hpp), the table e0_ck reads its first requests of a launch
// from: on synthetic layouts (random tile counts per workgroup and batch, empty lanes, workgroups with fewer tiles than
// wavefronts), every wavefront of every table shape is walked as the kernel walks it -- its number inside the group, the
// deal of the tiles of a round over the SIMDs (wave_t), tile_of -- and must find its first tile, that tile's header and the
// camera ranks of its first and second tile.  No HIP runtime call.
#include <cstdio>
#include <random>
#include <vector>

#include "../../povar_amd/csrc/ck_layout.hpp"

using namespace povar;

#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); return 1; } \
  } while (0)

static int check(int grid, int nb, unsigned seed) {
  std::mt19937 rng(seed);
  CkLayout K;
  K.nb = nb;
  K.bt_off.assign((size_t)grid * nb + 1, 0);
  int t = 0;
  for (int w = 0; w < grid; ++w)
    for (int b = 0; b < nb; ++b) {
      K.bt_off[(size_t)w * nb + b] = t;
      t += (int)(rng() % 40);  // 0 .. 39 tiles: none, fewer than a group's wavefronts, several rounds
    }
  K.bt_off[(size_t)grid * nb] = t;
  K.tile.resize(t);
  K.lane_cam.resize((size_t)t * WAVE);
  for (int i = 0; i < t; ++i) K.tile[i] = make_int4((int)(rng() % 100000), 1 + (int)(rng() % 16), (int)(rng() % 4), (int)(rng() % 50000));
  for (auto& r : K.lane_cam) r = rng() % 5 == 0 ? -1 : (int)(rng() % 65535);
  std::vector<int2> meta;
  std::vector<int4> hdr;
  ck_first_tables(K, grid, meta, hdr);
  CHECK(meta.size() == (size_t)CK_FIRST_PLANES * grid * 16 * WAVE && hdr.size() == (size_t)CK_FIRST_PLANES * grid * 16);
  int walked = 0, without = 0;
  for (int p = 0; p < CK_FIRST_PLANES; ++p) {
    const int gw = ck_first_gw(p), ng = ck_first_ng(p), nw = gw * ng;
    for (int w = 0; w < grid; ++w)
      for (int wave_all = 0; wave_all < nw; ++wave_all) {
        // (as e0_ck: povar_kernels_ck.hpp)
        const int grp = ng > 1 ? wave_all / gw : 0, wave = ng > 1 ? wave_all % gw : wave_all;
        const int wave_t = (wave & ~3) | (((wave >> 2) & 1) ? 3 - (wave & 3) : (wave & 3));
        auto tile_of = [&](int tb0, int q) { return tb0 + q * gw + ((q & 1) ? gw - 1 - wave_t : wave_t); };
        const size_t at = ((size_t)p * grid + w) * 16 + (size_t)(grp * gw + wave_t);
        if (grp >= nb) {
          for (int lane = 0; lane < WAVE; ++lane) CHECK(meta[at * WAVE + lane].y == -1);
          continue;
        }
        const int tb0 = K.bt_off[(size_t)w * nb + grp], tb1 = K.bt_off[(size_t)w * nb + grp + 1];
        const int t1 = tile_of(tb0, 0), t2 = tile_of(tb0, 1);
        for (int lane = 0; lane < WAVE; ++lane) {
          const int2 m = meta[at * WAVE + lane];
          if (t1 >= tb1) {
            CHECK(m.y == -1);
            continue;
          }
          const int r1 = m.x & 0xffff, r2 = (m.x >> 16) & 0xffff;
          CHECK(m.y == t1);
          CHECK((r1 == 0xffff ? -1 : r1) == K.lane_cam[(size_t)t1 * WAVE + lane]);
          if (t2 < tb1) CHECK((r2 == 0xffff ? -1 : r2) == K.lane_cam[(size_t)t2 * WAVE + lane]);
          else CHECK(r2 == 0xffff);
        }
        if (t1 < tb1) {
          const int4 a = hdr[at], e = K.tile[t1];
          CHECK(a.x == e.x && a.y == e.y && a.z == e.z && a.w == e.w);
          ++walked;
        } else {
          ++without;
        }
      }
  }
  CHECK(walked > 0 && without > 0);  // both paths of the kernel's prologue are covered
  return 0;
}

int main() {
  int rc = 0;
  rc |= check(7, 1, 1);
  rc |= check(13, 2, 2);
  rc |= check(5, 6, 3);
  if (rc == 0) std::printf("OK\n");
  return rc;
}
