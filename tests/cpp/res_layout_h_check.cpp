// Host-only check of the STEP-2 instance of the resident power series' layout (povar_amd/csrc/res_layout.hpp with
// res_shape_step2(): the layout of series_res_h): reads a problem dumped by tests/test_res_layout_joint.py, builds the
// layout, verifies the invariants series_res_h relies on -- those of res_layout_check.cpp, with the step-2 LDS formula
// written out here a second time and without image points -- and says whether step 1's cut of the same problem would
// serve step 2 as it is (res_shared_fits).  Plain C++17: no HIP header, no HIP runtime call.
// usage: res_layout_h_check n_cams lm_off.bin cam_idx.bin obs.bin W NW R HMIN HMAX LSMAX [force_order]
#include <cstdio>
#include <cstdlib>
#include <map>
#include <numeric>
#include <set>
#include <vector>

#include "../../povar_amd/csrc/res_layout.hpp"

using namespace povar;

template <class T>
static std::vector<T> read_vec(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v(n / sizeof(T));
  if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); return 1; } \
  } while (0)

// LDS of the fullest workgroup under the step-2 formula: control words, X and U4 / G4 at the slot capacity LS T of the
// instantiation (8 arrays of doubles), the region, per owned camera 121 + 12 + 13 + 11 + 11 + 12 + 2 + 60 doubles and four
// ints, the index lists
static size_t lds_step2(const ResLayout& R) {
  size_t worst = 0;
  for (int g = 0; g < R.W; ++g) {
    const size_t nC = R.cam_off[g + 1] - R.cam_off[g], nO = R.own_off[g + 1] - R.own_off[g], nQ = R.oq_off[g + 1] - R.oq_off[g];
    const size_t region = std::max(nC * 13, nQ * 12);
    const size_t b = 64 + (size_t)8 * 8 * R.LS * R.NW * 64 + region * 8 + nO * ((121 + 12 + 13 + 11 + 11 + 12 + 2 + 60) * 8 + 16) +
                     (nC + nQ) * 4 + 8;
    worst = std::max(worst, b);
  }
  return worst;
}

int main(int argc, char** argv) {
  if (argc < 11) return 2;
  const int n_cams = std::atoi(argv[1]), W = std::atoi(argv[5]), NW = std::atoi(argv[6]), RR = std::atoi(argv[7]),
            hmin = std::atoi(argv[8]), hmax = std::atoi(argv[9]), ls_max = std::atoi(argv[10]);
  const int force_order = argc > 11 ? std::atoi(argv[11]) : -1;
  const auto lm_off = read_vec<int32_t>(argv[2]);
  const auto cam_idx = read_vec<int32_t>(argv[3]);
  const auto obs = read_vec<double>(argv[4]);
  const int n_lms = (int)lm_off.size() - 1;
  const int64_t n_obs = lm_off[n_lms];
  std::vector<int64_t> cnt(n_cams, 0);
  for (int64_t i = 0; i < n_obs; ++i) cnt[cam_idx[i]]++;
  std::vector<int> order(n_cams), rank1(n_cams);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cnt[a] > cnt[b]; });
  for (int r = 0; r < n_cams; ++r) rank1[order[r]] = r + 1;
  std::vector<int> slot_of_obs(n_obs);
  for (int64_t i = 0; i < n_obs; ++i) slot_of_obs[i] = (int)(n_obs - 1 - i);  // any bijection: the layout only carries it
  // ---- step 1's cut of the same problem and shape: does it serve step 2 as it is?
  ResLayout R1;
  build_res(n_cams, n_lms, lm_off.data(), cam_idx.data(), obs.data(), rank1, slot_of_obs, W, NW, RR, hmin, hmax, ls_max, R1, force_order);
  const int fits1 = R1.fits ? 1 : 0;
  const size_t lds1_h = R1.fits ? lds_step2(R1) : 0;
  const int shared = res_shared_fits(R1) ? 1 : 0;
  CHECK(shared == (R1.fits && lds1_h <= (size_t)160 * 1024 ? 1 : 0));
  if (R1.fits) CHECK(res_lds_bytes_of(R1, res_shape_step2()) == lds1_h && R1.uv.size() == R1.lslot.size());
  // ---- the step-2 instance
  ResLayout R;
  build_res(n_cams, n_lms, lm_off.data(), cam_idx.data(), obs.data(), rank1, slot_of_obs, W, NW, RR, hmin, hmax, ls_max, R, force_order,
            res_shape_step2());
  if (!R.fits) {
    std::printf("{\"ok\": 1, \"fits\": 0, \"why\": \"%s\", \"max_lm\": %d, \"max_cam\": %d, \"fits1\": %d, \"shared\": %d, \"lds1_h\": %zu}\n",
                R.why, R.max_lm, R.max_cam, fits1, shared, lds1_h);
    return 0;
  }
  const int T = NW * WAVE, H = R.H;
  CHECK(R.W >= 1 && R.W <= RES_MAX_WG && R.W <= W && R.NW == NW && R.R == RR && H >= hmin && H <= hmax && (H & (H - 1)) == 0);
  CHECK((int)R.lm_off.size() == R.W + 1 && R.lm_off[R.W] == n_lms && (int)R.lm_id.size() == n_lms);
  CHECK((int)R.cam_off.size() == R.W + 1 && (int)R.cam_id.size() == R.cam_off[R.W] && R.cam_zi.size() == R.cam_id.size() && R.n_rec == R.cam_off[R.W]);
  const size_t n_pos = (size_t)R.W * RR * T;
  CHECK(R.lane_cam.size() == n_pos && R.lane_seg.size() == n_pos);
  CHECK(R.uv.empty());  // step 2 has no image points: neither built nor uploaded
  CHECK(R.lslot.size() == n_pos * H && R.oslot.size() == R.lslot.size());
  CHECK(R.wave_h.size() == (size_t)R.W * RR * NW);
  CHECK(R.LS >= 1 && R.LS <= ls_max && R.max_lm <= R.LS * T);
  CHECK(R.lds_bytes == lds_step2(R) && R.lds_bytes <= (size_t)160 * 1024);  // the STEP-2 formula
  // every landmark in exactly one slot, no empty range
  std::vector<int> lm_wg(n_lms, -1);
  int wg_without_owned = 0;
  for (int g = 0; g < R.W; ++g) {
    CHECK(R.lm_off[g + 1] > R.lm_off[g]);
    for (int s = R.lm_off[g]; s < R.lm_off[g + 1]; ++s) {
      CHECK(R.lm_id[s] >= 0 && R.lm_id[s] < n_lms && lm_wg[R.lm_id[s]] < 0);
      lm_wg[R.lm_id[s]] = g;
    }
  }
  // observations by (landmark, camera) -> index
  std::map<std::pair<int, int>, int64_t> where;
  for (int l = 0; l < n_lms; ++l)
    for (int i = lm_off[l]; i < lm_off[l + 1]; ++i) where[{l, cam_idx[i]}] = i;
  std::vector<char> seen(n_obs, 0);
  int64_t lanes_used = 0;
  for (int g = 0; g < R.W; ++g) {
    const int nC = R.cam_off[g + 1] - R.cam_off[g], nL = R.lm_off[g + 1] - R.lm_off[g];
    std::set<int> cams_of_wg;
    for (int s = 0; s < nC; ++s) {
      const int c = R.cam_id[R.cam_off[g] + s];
      CHECK(c >= 0 && c < n_cams && cams_of_wg.insert(c).second && R.cam_zi[R.cam_off[g] + s] == rank1[c] - 1);
      if (s > 0) CHECK(rank1[c] > rank1[R.cam_id[R.cam_off[g] + s - 1]]);  // most observed first
    }
    std::map<int, int> runs_of_slot, single_flag;
    for (int r = 0; r < RR; ++r)
      for (int wv = 0; wv < NW; ++wv) {
        const int wh = R.wave_h[((size_t)g * RR + r) * NW + wv], hrows = wh & 255, dup = (wh >> 8) & 1, steps = (wh >> 12) & 15;
        CHECK(hrows <= H && steps >= 1 && steps <= 4);
        bool any_dup = false;
        for (int l = 0; l < WAVE; ++l) {
          const size_t t = (size_t)wv * WAVE + l, lane = ((size_t)g * RR + r) * T + t;
          const int ci = R.lane_cam[lane];
          if (ci < 0) {
            for (int j = 0; j < H; ++j) CHECK(R.lslot[(((size_t)g * RR + r) * H + j) * T + t] < 0);
            continue;
          }
          ++lanes_used;
          CHECK(ci < nC);
          const int cam = R.cam_id[R.cam_off[g] + ci];
          const int s0 = R.lane_seg[lane] & 255, s1 = (R.lane_seg[lane] >> 8) & 255;
          CHECK(s0 <= l && l <= s1 && s1 < WAVE);
          const size_t base = ((size_t)g * RR + r) * T + (size_t)wv * WAVE;
          for (int q = s0; q <= s1; ++q) CHECK(R.lane_cam[base + q] == ci && R.lane_seg[base + q] == R.lane_seg[lane]);
          single_flag[ci] = (R.lane_seg[lane] >> 16) & 1;
          if (s0 > 0) CHECK(R.lane_cam[base + s0 - 1] != ci);
          if (s1 + 1 < WAVE) CHECK(R.lane_cam[base + s1 + 1] != ci);
          if (l == s0) runs_of_slot[ci]++;
          if (s1 > s0) { any_dup = true; CHECK((1 << steps) >= std::min(s1 - s0 + 1, 16)); }
          bool ended = false;
          for (int j = 0; j < H; ++j) {
            const size_t row = (((size_t)g * RR + r) * H + j) * T + t;
            if (R.lslot[row] < 0) { ended = true; continue; }
            CHECK(!ended && j < hrows && R.lslot[row] % 3 == 0);  // (3 x slot: the convention of step 1's rows, which step 2 may share)
            const int slot = R.lslot[row] / 3;
            CHECK(slot < nL && slot < R.LS * T);  // inside the workgroup AND inside the compile-time stride of the LDS arrays
            const int lm = R.lm_id[R.lm_off[g] + slot];
            auto it = where.find({lm, cam});
            CHECK(it != where.end());  // the slot names the observation's landmark, the chunk its camera
            const int64_t i = it->second;
            CHECK(!seen[i]);
            seen[i] = 1;
            CHECK(R.oslot[row] == slot_of_obs[i]);
          }
        }
        CHECK(any_dup == (dup != 0));
      }
    CHECK((int)runs_of_slot.size() == nC);  // every camera slot of the workgroup has a chunk
    for (auto& kv : runs_of_slot) CHECK(single_flag[kv.first] == (kv.second == 1 ? 1 : 0));
  }
  for (int64_t i = 0; i < n_obs; ++i) CHECK(seen[i]);
  // owners: every camera once; its records = the slots that name it, each once, camera-major in workgroup order
  CHECK((int)R.own_off.size() == R.W + 1 && R.own_off[R.W] == n_cams && (int)R.own_cam.size() == n_cams);
  CHECK((int)R.oq_off.size() == R.W + 1 && R.oq_off[R.W] == R.n_rec && (int)R.oq_rec.size() == R.n_rec);
  CHECK(R.own_q.size() == R.own_cam.size() && R.own_zi.size() == R.own_cam.size());
  std::vector<int> owned(n_cams, 0), rec_seen(R.n_rec, 0);
  for (int g = 0; g < R.W; ++g) {
    int q = 0;
    if (R.own_off[g + 1] == R.own_off[g]) ++wg_without_owned;
    for (int o = R.own_off[g]; o < R.own_off[g + 1]; ++o) {
      const int c = R.own_cam[o];
      CHECK(c >= 0 && c < n_cams && owned[c]++ == 0 && R.own_zi[o] == rank1[c] - 1);
      CHECK(R.own_q[o].x == q && R.own_q[o].y >= q);
      int prev = -1;
      for (q = R.own_q[o].x; q < R.own_q[o].y; ++q) {
        const int rec = R.oq_rec[(size_t)R.oq_off[g] + q];
        CHECK(rec >= 0 && rec < R.n_rec && rec_seen[rec]++ == 0 && R.cam_id[rec] == c && rec > prev);
        prev = rec;
      }
    }
    CHECK(q == R.oq_off[g + 1] - R.oq_off[g]);
  }
  for (int c = 0; c < n_cams; ++c) CHECK(owned[c] == 1);
  for (int r = 0; r < R.n_rec; ++r) CHECK(rec_seen[r] == 1);
  std::printf("{\"ok\": 1, \"fits\": 1, \"W\": %d, \"H\": %d, \"LS\": %d, \"order\": %d, \"n_rec\": %d, \"max_lm\": %d, \"max_cam\": %d, "
              "\"max_oq\": %d, \"max_own\": %d, \"max_chunks\": %d, \"lanes_used\": %lld, \"wg_without_owned\": %d, \"lds_bytes\": %zu, "
              "\"fits1\": %d, \"shared\": %d, \"lds1_h\": %zu, \"lds1\": %zu}\n",
              R.W, H, R.LS, R.order, R.n_rec, R.max_lm, R.max_cam, R.max_oq, R.max_own, R.max_chunks, (long long)lanes_used,
              wg_without_owned, R.lds_bytes, fits1, shared, lds1_h, R1.fits ? R1.lds_bytes : (size_t)0);
  return 0;
}
