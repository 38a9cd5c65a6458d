// ch_gather_plan.hpp — the lane schedule of the one-wave gather (pure C++, no HIP): which lane of the wavefront sums which stamp
// sources in which trip, and where the sums go.  Built once per block class from the class's gather lists (mat_ptr / vec_ptr over
// mat_src | vec_src, ch_analysis.hpp); read per Newton iteration by tran_persistent_kernel (ch_persist.hpp).
//
// The work list of class_blobs (ch_engine.hip) hands item w to lane w % 64 and lets every lane loop over its item's sources: the
// wave runs as many trips as its heaviest item needs, a second pass for items 64 .. 127, and every lane keeps its own loop state
// under an exec mask.  Here the items (one per structural non-zero of A / C, per diagonal and per row of F / Q) are PACKED onto the
// 64 lanes, heaviest first, an item's four-source trips consecutive in one lane, several items one after another in a lane, so that
// the wave runs T trips in all — T = the heaviest lane — and a trip is the same straight-line code in every lane:
//
//   A lane's trips are consecutive RECORDS; record 0 is the idle trip every lane reads once its own list is done.  The table
//   (ints; it lies directly behind the class blob, ClassMeta::spare0 = its length, spare1 = T):
//     head[64]    per lane: first record | records << 16
//     src[R]      8 bytes per record: four uint16 staging offsets (sources 4q .. 4q+3 of the lane's current item, in list order; unused 0)
//     ctl[R]      4 bytes per record (R = 1 + all trips, rounded up to a multiple of 4):
//                 bits 0..2  number of valid sources (0: the idle record, or the close of an item that has no source at all)
//                 bit  3     the item ends in this trip: its sums are stored and the lane's accumulators start again from zero
//                 bit  4     the item is a row of F / Q (second addend at the charge offset; F, Q and the right-hand side are written)
//                 bits 6..18  offset (doubles) of the item's entry from A:  r * lda + col  |  e * lda + lda - 1 (the right-hand side column)
//                 bits 19..31 offset (doubles) from Cm:  r * ldc + col  |  nc * ldc + 3 * nc + e = Qv[e]  (Fv[e] one row of nc below,
//                             hq[e] one above: the wave region keeps xl xp F Q hq in this order behind Cm's nc rows)
//   lda / ldc are the row strides of the two images.  Unpadded (newton_block_kernel's layout, and the bordered form of the device
//   stepper): nc + 1 / nc.  Padded (every other form of the device stepper, GatherStrides below): NC + 1 / NC for the register-LU
//   size NC the kernel is instantiated with; the entries of the pad rows and pad columns are no item's destination.
//   A dense [T][64] table would be simpler to index, but one heavy item (the rail diagonal of a torn array: 15 trips) would make
//   every lane pay its length in LDS; this form costs 12 bytes per trip in use.
// The sums themselves are what they were: every item's sources are added in list order, in one lane, starting from 0.0.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

namespace chip {

constexpr int GP_HEAD_INTS = 64;    // per lane: first record | records << 16
constexpr unsigned GP_N_MASK = 7u, GP_END = 8u, GP_VEC = 16u;
constexpr int GP_A_SHIFT = 6, GP_C_SHIFT = 19;
constexpr unsigned GP_OFS_MASK = 0x1fffu;

// Register-LU size of the tran_persistent_kernel instantiation a circuit runs (ch_engine_persist.hpp persist_pick_kernel), 0 when
// it has none, and the strides of its LDS images of A and C: padded to NC except in the bordered form, which keeps its guarded
// solve and the unpadded images.
inline int persist_lu_nc(bool wide, int nb, int max_nc) { return max_nc > 16 ? 0 : ((wide || nb > 0 || max_nc > 12) ? 16 : 12); }
struct GatherStrides {
  int lda, ldc;
  static GatherStrides unpadded(int nc) { return {nc + 1, nc}; }
  static GatherStrides of(bool wide, int nb, int max_nc, int nc) {
    const int NC = persist_lu_nc(wide, nb, max_nc);
    return (NC == 0 || nb > 0 || nc > NC) ? unpadded(nc) : GatherStrides{NC + 1, NC};
  }
  bool padded(int nc) const { return lda != nc + 1; }
  // doubles the two images take beyond their unpadded size (A has lda - 1 rows when padded, C always nc)
  int extra_doubles(int nc) const { return padded(nc) ? (lda - 1) * lda + nc * ldc - nc * (nc + 1) - nc * nc : 0; }
};

struct GatherPlan {
  struct Item { int first, cnt, code; };   // first source (index into mat_src | vec_src), sources, entry | 0x8000 for a row of F / Q
  int T = 0;                       // trips of the wave
  int n_items = 0, total_trips = 0, max_item_trips = 0;
  int R = 0;                       // records: the idle one + every trip, rounded up to a multiple of 4
  std::vector<int> words;          // head[64] | src[2 R] | ctl[R]
  std::vector<int> item_lane, item_trip;   // where every item starts (for the tests); items in work-list order
  std::vector<Item> items;

  static int trips_of(int cnt) { return cnt <= 0 ? 1 : (cnt + 3) / 4; }
  static int lower_bound_T(int total_trips, int max_item_trips) { return std::max((total_trips + 63) / 64, max_item_trips); }

  // the items of a class in the order of the work list: rows of F / Q first, then the structural non-zeros and every diagonal,
  // stably sorted by descending source count
  static std::vector<Item> class_items(int nc, const std::vector<int>& mat_ptr, const std::vector<int>& vec_ptr, int n_mat_src) {
    std::vector<Item> it;
    for (int i = 0; i < nc; ++i) it.push_back({n_mat_src + vec_ptr[i], vec_ptr[i + 1] - vec_ptr[i], (int)(0x8000u | (uint32_t)i)});
    for (int e = 0; e < nc * nc; ++e) {
      const int cnt = mat_ptr[e + 1] - mat_ptr[e];
      if (cnt == 0 && e / nc != e % nc) continue;
      it.push_back({mat_ptr[e], cnt, e});
    }
    std::stable_sort(it.begin(), it.end(), [](const Item& x, const Item& y) { return x.cnt > y.cnt; });
    return it;
  }

  // src16 = mat_src | vec_src.  false: the class does not fit the one-wave path (nc > 64, or no lists)
  bool build(int nc, const std::vector<int>& mat_ptr, const std::vector<int>& vec_ptr, const std::vector<uint16_t>& src16, int n_mat_src) {
    return build(nc, mat_ptr, vec_ptr, src16, n_mat_src, GatherStrides::unpadded(nc));
  }
  bool build(int nc, const std::vector<int>& mat_ptr, const std::vector<int>& vec_ptr, const std::vector<uint16_t>& src16, int n_mat_src, GatherStrides gs) {
    T = 0; R = 0; n_items = 0; total_trips = 0; max_item_trips = 0; words.clear(); item_lane.clear(); item_trip.clear(); items.clear();
    if (nc < 1 || nc > 64 || (int)vec_ptr.size() != nc + 1 || (int)mat_ptr.size() != nc * nc + 1) return false;
    if (gs.lda <= nc || gs.ldc < nc) return false;
    items = class_items(nc, mat_ptr, vec_ptr, n_mat_src);
    n_items = (int)items.size();
    for (const Item& it : items) { total_trips += trips_of(it.cnt); max_item_trips = std::max(max_item_trips, trips_of(it.cnt)); }
    // first fit, heaviest first, into 64 lanes of T trips; T from its lower bound upwards.  First fit places an item of s trips unless
    // every lane holds more than T - s, so it succeeds at the latest with T = ceil(total / 64) + heaviest - 1.
    std::vector<int> order(n_items);
    for (int i = 0; i < n_items; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return trips_of(items[x].cnt) > trips_of(items[y].cnt); });
    std::array<int, 64> load;
    for (int t = lower_bound_T(total_trips, max_item_trips);; ++t) {
      load.fill(0);
      item_lane.assign(n_items, -1); item_trip.assign(n_items, 0);
      bool ok = true;
      for (int i : order) {
        const int s = trips_of(items[i].cnt);
        int l = 0;
        while (l < 64 && load[l] + s > t) ++l;
        if (l == 64) { ok = false; break; }
        item_lane[i] = l; item_trip[i] = load[l]; load[l] += s;
      }
      if (ok) { T = t; break; }
    }
    // records: lane by lane, a lane's items in the order they were placed (item_trip = trip inside the lane)
    std::array<int, 64> base;
    { int next = 1; for (int l = 0; l < 64; ++l) { base[l] = load[l] > 0 ? next : 0; next += load[l]; } R = (next + 3) & ~3; }
    const int lda = gs.lda, ldc = gs.ldc;
    words.assign((size_t)GP_HEAD_INTS + 3 * (size_t)R, 0);
    int* src = words.data() + GP_HEAD_INTS; int* ctl = src + 2 * (size_t)R;
    for (int l = 0; l < 64; ++l) words[l] = (int)((uint32_t)base[l] | ((uint32_t)load[l] << 16));
    for (int i = 0; i < n_items; ++i) {
      const Item& it = items[i];
      const int l = item_lane[i], s = trips_of(it.cnt);
      const bool vec = (it.code & 0x8000) != 0;
      const int e = it.code & 0x7fff;
      const unsigned oa = vec ? (unsigned)(e * lda + lda - 1) : (unsigned)((e / nc) * lda + e % nc);
      const unsigned oc = vec ? (unsigned)(nc * ldc + 3 * nc + e) : (unsigned)((e / nc) * ldc + e % nc);
      for (int q = 0; q < s; ++q) {
        const int rec = base[l] + item_trip[i] + q;
        const int left = it.cnt - 4 * q, n = left < 0 ? 0 : (left > 4 ? 4 : left);
        uint16_t o[4] = {0, 0, 0, 0};
        for (int k = 0; k < n; ++k) o[k] = src16[(size_t)it.first + 4 * q + k];
        src[2 * rec] = (int)((uint32_t)o[0] | ((uint32_t)o[1] << 16));
        src[2 * rec + 1] = (int)((uint32_t)o[2] | ((uint32_t)o[3] << 16));
        unsigned c = (unsigned)n | (vec ? GP_VEC : 0u);
        if (q == s - 1) c |= GP_END | (oa << GP_A_SHIFT) | (oc << GP_C_SHIFT);
        ctl[rec] = (int)c;
      }
    }
    if ((unsigned)(nc * lda) > GP_OFS_MASK || (unsigned)(nc * ldc + 4 * nc) > GP_OFS_MASK) return false;   // (64 * 65: the offsets always fit)
    if (R > 0xffff || T > 0xffff) return false;   // (far beyond what 16-bit staging offsets let a class hold)
    return true;
  }
};

}  // namespace chip
