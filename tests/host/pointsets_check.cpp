// pointsets_check.cpp -- csrc/pointsets.h on the host: the SetDesc builder, the block starts, the one assembler and the input
// map, each against a direct statement of what it has to give.  Built with -fsanitize=address,undefined by
// tests/test_pointsets_host.py, so a write outside a buffer ends the program even where no CHECK looks.  Needs no GPU and no HIP.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pinns-tf2.0_amd/csrc/pointsets.h"

using namespace pinn;

static long g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      if (g_failed < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed += 1;                                                                         \
    }                                                                                        \
  } while (0)

template <typename T>
static bool same_bits(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }

// Entry (row, col) of input `which` of member k: every value is its own, none is 0, GUARD or a coordinate of LB
enum { IN_LO = 1, IN_HI, IN_XU, IN_U, IN_XF };
static double val(int k, int which, int row, int col) { return 100000.0 * (k + 1) + 1000.0 * which + row + 0.25 * col + 0.5; }
static const double LB[2] = {-7.5, 3.25};
static const double GUARD = -12345.678;
static const int N_GUARD = 8, K = 3;

static PointSets member_sets(int k, int n_b, int n_u, int n_f, int n_out, bool device_colloc) {
  PointSets ps;
  for (int i = 0; i < n_b; ++i)
    for (int j = 0; j < 2; ++j) { ps.Xlo.push_back(val(k, IN_LO, i, j)); ps.Xhi.push_back(val(k, IN_HI, i, j)); }
  for (int i = 0; i < n_u; ++i) {
    for (int j = 0; j < 2; ++j) ps.Xu.push_back(val(k, IN_XU, i, j));
    for (int o = 0; o < n_out; ++o) ps.U.push_back(val(k, IN_U, i, o));
  }
  if (!device_colloc)                               // (a device origin keeps no host points)
    for (int i = 0; i < n_f; ++i)
      for (int j = 0; j < 2; ++j) ps.Xf.push_back(val(k, IN_XF, i, j));
  return ps;
}

// the layout, stated directly: coordinate j of point g of member k's set, and its target for output o
static double want_coord(int k, int g, int j, int n_b, int n_u, int n_f, bool interleaved, bool device_colloc) {
  if (g < 2 * n_b) {
    const bool hi = interleaved ? (g & 1) : g >= n_b;
    const int row = interleaved ? g / 2 : (hi ? g - n_b : g);
    return val(k, hi ? IN_HI : IN_LO, row, j);
  }
  g -= 2 * n_b;
  if (g < n_u) return val(k, IN_XU, g, j);
  g -= n_u;
  if (g < n_f && !device_colloc) return val(k, IN_XF, g, j);
  return LB[j];                                     // a placeholder of the device's block, the Robin block's slots, padding
}
static double want_target(int k, int g, int o, int n_b, int n_u) {
  const int row = g - 2 * n_b;
  return row >= 0 && row < n_u ? val(k, IN_U, row, o) : 0.0;
}

static void one_shape(int n_b, int n_u, int n_f, int n_w, int n_out, bool interleaved, bool device_colloc) {
  g_cases += 1;
  const int64_t tot_b = n_b ? n_b + 3 : 0, tot_u = n_u ? 2 * n_u : 0, tot_f = n_f ? 7 * (int64_t)n_f + 1 : 0;
  const SetDesc sd = make_set_desc(n_b, n_u, n_f, tot_b, tot_u, tot_f, n_w);
  CHECK(sd.n_b == n_b && sd.n_u == n_u && sd.n_f == n_f && sd.n_all == 2 * n_b + n_u + n_f);
  CHECK(sd.n_pad % 64 == 0 && sd.n_pad >= sd.n_all + n_w && sd.n_pad - (sd.n_all + n_w) < 64);
  CHECK(same_bits(sd.inv_nb, tot_b ? 1.0 / (double)tot_b : 0.0));
  CHECK(same_bits(sd.inv_nu, tot_u ? 1.0 / (double)tot_u : 0.0));
  CHECK(same_bits(sd.inv_nf, tot_f ? 1.0 / (double)tot_f : 0.0));
  CHECK(data_first(sd) == 2 * n_b && colloc_first(sd) == 2 * n_b + n_u && robin_first(sd) == 2 * n_b + n_u + n_f);

  // K members into adjacent slices of one block each, guards in front and behind; nothing is pre-set to a wanted value
  const size_t n_pad = sd.n_pad;
  std::vector<double> x(K * n_pad + 2 * N_GUARD, GUARD), t(x), tg((size_t)K * n_out * n_pad + 2 * N_GUARD, GUARD);
  for (int k = 0; k < K; ++k) {
    const PointSets ps = member_sets(k, n_b, n_u, n_f, n_out, device_colloc);
    CHECK(has_counts(ps, sd, n_out, device_colloc));
    assemble_set(ps, sd, n_out, interleaved, device_colloc, LB, x.data() + N_GUARD + k * n_pad, t.data() + N_GUARD + k * n_pad,
                 tg.data() + N_GUARD + (size_t)k * n_out * n_pad);
  }
  for (int i = 0; i < N_GUARD; ++i) {
    CHECK(x[i] == GUARD && t[i] == GUARD && tg[i] == GUARD);
    CHECK(x[x.size() - 1 - i] == GUARD && t[t.size() - 1 - i] == GUARD && tg[tg.size() - 1 - i] == GUARD);
  }
  for (int k = 0; k < K; ++k) {                     // after all K calls: a write into a neighbour's slice shows here
    const double *xk = x.data() + N_GUARD + k * n_pad, *tk = t.data() + N_GUARD + k * n_pad;
    const double* tgk = tg.data() + N_GUARD + (size_t)k * n_out * n_pad;
    for (int g = 0; g < sd.n_pad; ++g) {
      CHECK(xk[g] == want_coord(k, g, 0, n_b, n_u, n_f, interleaved, device_colloc));
      CHECK(tk[g] == want_coord(k, g, 1, n_b, n_u, n_f, interleaved, device_colloc));
      for (int o = 0; o < n_out; ++o) CHECK(tgk[(size_t)o * n_pad + g] == want_target(k, g, o, n_b, n_u));
      if (g >= sd.n_all) CHECK(xk[g] == LB[0] && tk[g] == LB[1]);
    }
    if (interleaved)                                // the partner of pair point g is g ^ 1: the other wall's point of the same row
      for (int g = 0; g < 2 * n_b; ++g) {
        CHECK(xk[g] == val(k, (g & 1) ? IN_HI : IN_LO, g / 2, 0));
        CHECK(xk[g ^ 1] == val(k, (g & 1) ? IN_LO : IN_HI, g / 2, 0));
      }
  }
}

static void builder_reciprocals() {
  const SetDesc z = make_set_desc(1, 1, 1, 0, 0, 0, 0);
  CHECK(same_bits(z.inv_nb, 0.0) && same_bits(z.inv_nu, 0.0) && same_bits(z.inv_nf, 0.0));
  const SetDesc s = make_set_desc(1, 1, 1, 7, 11, 13, 0);
  CHECK(same_bits(s.inv_nb, 1.0 / 7.0) && same_bits(s.inv_nu, 1.0 / 11.0) && same_bits(s.inv_nf, 1.0 / 13.0));
  CHECK(make_set_desc(0, 0, 64, 0, 0, 64, 0).n_pad == 64 && make_set_desc(0, 0, 64, 0, 0, 64, 1).n_pad == 128);
  CHECK(make_set_desc(0, 1, 0, 0, 1, 0, 0).n_pad == 64 && make_set_desc(7, 63, 70, 7, 63, 70, 3).n_pad == 192);
}

// the members' store: a broadcast gives every entry the same rows, a slice gives entry k row k; a set that is one value short
// of the counts is seen
static void store_helpers() {
  std::vector<PointSets> sets(K);
  const double v[6] = {1, 2, 3, 4, 5, 6};
  broadcast_field(sets, &PointSets::Xu, v, 2);
  for (int k = 0; k < K; ++k) CHECK(sets[k].Xu.size() == 2 && sets[k].Xu[0] == 1 && sets[k].Xu[1] == 2 && sets[k].Xf.empty());
  slice_field(sets, &PointSets::U, v, 2);
  for (int k = 0; k < K; ++k) CHECK(sets[k].U.size() == 2 && sets[k].U[0] == v[2 * k] && sets[k].U[1] == v[2 * k + 1]);
  broadcast_field(sets, &PointSets::Xu, nullptr, 0);
  for (int k = 0; k < K; ++k) CHECK(sets[k].Xu.empty());
  const SetDesc sd = make_set_desc(1, 1, 1, 1, 1, 1, 0);
  for (PointField f : {&PointSets::Xf, &PointSets::Xu, &PointSets::U, &PointSets::Xlo, &PointSets::Xhi}) {
    PointSets ps = member_sets(0, 1, 1, 1, 2, false);
    CHECK(has_counts(ps, sd, 2, false));
    (ps.*f).pop_back();
    CHECK(!has_counts(ps, sd, 2, false));
    CHECK(has_counts(ps, sd, 2, true) == (f == &PointSets::Xf));      // (a device origin does not count host points)
  }
}

// the four boxes of tests/helpers/boxes.py, both compute types, bit for bit against the expressions every launch used
template <typename real>
static void input_map() {
  const double boxes[4][2][2] = {{{0.25, 0.5}, {1.75, 2.0}}, {{-3.0, -2.0}, {-2.4, -0.7}}, {{3.0, 10.0}, {3.5, 12.0}},
                                 {{100.0, -50.0}, {101.0, -49.0}}};
  for (const auto& box : boxes) {
    const double *lb = box[0], *ub = box[1];
    const InMap<real> m(lb, ub);
    CHECK(same_bits(m.lbx, (real)lb[0]) && same_bits(m.lbt, (real)lb[1]));
    CHECK(same_bits(m.sx, (real)(2.0 / (ub[0] - lb[0]))) && same_bits(m.st, (real)(2.0 / (ub[1] - lb[1]))));
    CHECK(same_bits(m.ex, ub[0] - lb[0]) && same_bits(m.et, ub[1] - lb[1]));
  }
}

int main() {
  for (int n_b : {0, 1, 7})
    for (int n_u : {0, 1, 63})
      for (int n_f : {0, 1, 64, 70})
        for (int n_w : {0, 3})
          for (int n_out : {1, 2})
            for (int interleaved = 0; interleaved < 2; ++interleaved)
              for (int device_colloc = 0; device_colloc < 2; ++device_colloc)
                if (2 * n_b + n_u + n_f > 0)        // (the engine refuses the empty set before it assembles)
                  one_shape(n_b, n_u, n_f, n_w, n_out, interleaved != 0, device_colloc != 0);
  builder_reciprocals();
  store_helpers();
  input_map<double>();
  input_map<float>();
  if (g_failed) { fprintf(stderr, "pointsets_check: %ld checks failed\n", g_failed); return 1; }
  printf("pointsets_check ok (%ld shapes, %d members each)\n", g_cases, K);
  return 0;
}
