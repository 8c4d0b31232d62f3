// optim_host_check.cpp -- csrc/optim_host.h on the host: the ticket counters, Adam's step factors against the expression the
// engine used to write out, the loss ring's layout, and the L-BFGS log window / hand-out against a model of the device's
// logging, swept exhaustively.  Built with -fsanitize=address,undefined by tests/test_optim_host.py, so a read outside a
// window ends the program even where no CHECK looks.  Needs no GPU and no HIP.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../pinns-tf2.0_amd/csrc/optim_host.h"

using namespace pinn;

static long g_failed = 0;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      if (g_failed < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed += 1;                                                                         \
    }                                                                                        \
  } while (0)

// ---- tickets ---------------------------------------------------------------------------------------------------------------
static void check_tickets() {
  static_assert(N_PENDING == 4, "the C API documents 4 chunks in flight");
  Tickets tk;
  tk.issued = tk.collected = (1ull << 31) - 3;      // the numbers wrap to 0 three tickets on
  CHECK(tk.outstanding() == 0 && tk.room() && !tk.is_oldest(tk.next_number()));
  std::vector<int> number, slot;                    // of every ticket issued, in order
  size_t collected = 0;
  auto issue = [&] {
    number.push_back(tk.next_number());
    slot.push_back(tk.next_slot());
    tk.issued += 1;
  };
  auto collect = [&] {
    CHECK(tk.is_oldest(number[collected]));
    CHECK(tk.oldest_slot() == slot[collected]);     // the slot of a ticket is the slot it was issued into
    for (size_t j = collected + 1; j < number.size(); ++j) CHECK(!tk.is_oldest(number[j]));   // in order only
    tk.collected += 1;
    collected += 1;
  };
  for (int round = 0; round < 6; ++round) {         // fill to 4, take `round % 4 + 1` back, fill again ...
    while (tk.room()) issue();
    CHECK(tk.outstanding() == N_PENDING);
    for (size_t a = collected; a < number.size(); ++a)       // the chunks in flight sit in different slots
      for (size_t b = a + 1; b < number.size(); ++b) CHECK(slot[a] != slot[b]);
    for (int j = 0; j <= round % 4; ++j) collect();
  }
  while (tk.outstanding() > 0) collect();
  CHECK(!tk.is_oldest(number.back()) && !tk.is_oldest(tk.next_number()));
  for (size_t i = 0; i < number.size(); ++i) {
    CHECK(number[i] >= 0);
    CHECK(number[i] == (int)((((1ull << 31) - 3) + i) & 0x7fffffff));
  }
  CHECK(number[2] == 0x7fffffff && number[3] == 0 && number.size() > 8);
  issue(); issue();
  tk.drop_all();
  CHECK(tk.outstanding() == 0 && tk.room());
}

// ---- Adam ------------------------------------------------------------------------------------------------------------------
static void check_adam() {
  volatile double vb1 = 0.9, vb2 = 0.999;           // (volatile: nothing is folded at compile time)
  const double lrs[3] = {1e-3, 0.03, 0.8};
  for (int it = 1; it <= 2000; ++it) {
    const double b1 = vb1, b2 = vb2, t = (double)it;
    const AdamFactors f(b1, b2, t);
    for (double lr_ : lrs) {
      volatile double vlr = lr_;
      const double lr = vlr;
      // the step size and the bare correction as adam_issue wrote them out before this header existed
      const double alpha = lr * std::sqrt(1.0 - std::pow(b2, t)) / (1.0 - std::pow(b1, t));
      const double bc_pw = std::sqrt(1.0 - std::pow(b2, t)) / (1.0 - std::pow(b1, t));
      CHECK(f.alpha(lr) == alpha);
      CHECK(f.bc_pw() == bc_pw);
    }
  }
}

// ---- Adam's loss ring --------------------------------------------------------------------------------------------------------
static void check_ring() {
  CHECK(ring_steps(0) == 16 && ring_steps(1) == 16 && ring_steps(16) == 16 && ring_steps(17) == 17 && ring_steps(5000) == 5000);
  CHECK(ring_doubles(16) == 16 * 4 * 3);
  CHECK(ring_must_grow(16, 0) && ring_must_grow(16, 16 * 4 * 3 * 8 - 1) && !ring_must_grow(16, 16 * 4 * 3 * 8));
  CHECK(ring_must_grow(17, 16 * 4 * 3 * 8) && !ring_must_grow(16, 17 * 4 * 3 * 8));
  Tickets tk;
  tk.issued = tk.collected = 1234567;
  for (size_t stride : {(size_t)16, (size_t)300}) {
    std::vector<size_t> start;                      // the regions of four chunks in flight: apart by a stride, inside the ring
    for (int j = 0; j < N_PENDING; ++j) { start.push_back(ring_region(tk, stride)); tk.issued += 1; }
    for (int a = 0; a < N_PENDING; ++a) {
      CHECK(start[a] % (3 * stride) == 0 && start[a] + 3 * stride <= ring_doubles(stride));
      CHECK(start[a] == (size_t)((1234567 + a) % 4) * stride * 3);
      for (int b = a + 1; b < N_PENDING; ++b) CHECK(start[a] != start[b]);
    }
    tk.collected = tk.issued;
  }
}

// ---- the L-BFGS log ----------------------------------------------------------------------------------------------------------
// The device as the host's arithmetic has to assume it: iteration i = 1 .. max_iter, each but the max_iter-th followed by one
// evaluation; evaluation i logs an entry when bit i - 1 of `pattern` is set (0 or 1 entry each), unless the run has broken:
// evaluation `brk` ends it without an entry and nothing is logged afterwards (brk = 0: no break).  The stream is in order, so
// the state and the window a chunk copies at its close see every evaluation issued so far.
struct Device {
  int max_iter, brk;
  unsigned pattern;
  bool done = false;
  std::vector<int> log;                             // the evaluations that logged, in order; max_iter + 1 entries of room
  int room() const { return max_iter + 1; }
  void evaluation(int i) {
    if (done) return;
    if (i == brk) { done = true; return; }
    if (pattern >> (i - 1) & 1u) log.push_back(i);
  }
};

struct Chunk { int n = 0, base = 0, issued_upto = 0, n_logged = 0, asked = 0; std::vector<int> h_iter; };

struct Sweep {
  long runs = 0, collects = 0, entries = 0;
  int slack_min = 1 << 30;                          // least (window - entries the window had to cover) over unclipped windows
  int sync_fresh_max[7] = {0, 0, 0, 0, 0, 0, 0};    // per chunk size: most entries one synchronous call handed out
};

// one run: chunks of n_iters, the host `lag` chunks behind (0: pinn_lbfgs_run, collect at once), until every iteration is
// issued, then one chunk more (the one that sees done one chunk late), then everything collected
static void run_model(int max_iter, int n_iters, int lag, unsigned pattern, int brk, Sweep& sw) {
  Device dev{max_iter, brk, pattern, false, {}};
  Tickets tk;
  Chunk pend[N_PENDING];
  int iters_issued = 0, issued_at_read = 0, logged_read = 0;        // the host's side (pinn_ctx::lbfgs)
  int handed = 0, uncollected = 0;                                  // entries handed out; iterations asked for and not collected
  sw.runs += 1;

  auto enqueue = [&] {
    CHECK(tk.room());
    Chunk& p = pend[tk.next_slot()];
    const int window = lbfgs_window(iters_issued, issued_at_read, n_iters, dev.room(), logged_read, max_iter);
    {  // the window as pinn's lbfgs_open wrote it out before this header existed
      int w = (iters_issued - issued_at_read) + n_iters + 1;
      if (w > dev.room() - logged_read) w = dev.room() - logged_read;
      if (w < 0 || max_iter == 0) w = 0;
      CHECK(window == w);
    }
    p.asked = n_iters;
    uncollected += n_iters;
    if (max_iter == 0) { p.n = -1; tk.issued += 1; return; }         // done at once, nothing copied
    const bool clipped = window != (iters_issued - issued_at_read) + n_iters + 1;
    for (int s = 0; s < n_iters && iters_issued < max_iter; ++s) {
      iters_issued += 1;
      if (iters_issued == max_iter) break;                           // last iteration: no re-evaluation
      dev.evaluation(iters_issued);
    }
    p.n = window; p.base = logged_read; p.issued_upto = iters_issued;
    p.n_logged = (int)dev.log.size();
    CHECK(p.base + window <= dev.room());                            // the copy stays inside the device's log arrays
    p.h_iter.assign((size_t)window, -1);                             // what the log held at the close; -1: not written yet
    for (int j = 0; j < window && p.base + j < (int)dev.log.size(); ++j) p.h_iter[j] = dev.log[p.base + j];
    if (!clipped) sw.slack_min = std::min(sw.slack_min, window - (p.n_logged - p.base));
    tk.issued += 1;
  };

  auto collect = [&] {
    CHECK(tk.outstanding() > 0);
    const Chunk& p = pend[tk.oldest_slot()];
    tk.collected += 1;
    sw.collects += 1;
    const int cap_async = uncollected + 1;                           // Engine.lbfgs_collect
    uncollected -= p.asked;
    if (p.n < 0) { CHECK(max_iter == 0); return; }
    const LbfgsHandout h = lbfgs_handout(p.n_logged, logged_read, p.base, p.n);
    CHECK(h.inside);
    CHECK(h.fresh >= 0 && h.fresh <= cap_async);
    if (lag == 0) {                                                  // pinn_lbfgs_run, Engine / Ensemble.lbfgs_run
      CHECK(h.fresh <= n_iters);                                     // the bound include/pinn_hip.h states
      CHECK(h.fresh <= std::max(n_iters, 1) && h.fresh <= n_iters + 1);   // the wrappers' arrays
      sw.sync_fresh_max[n_iters] = std::max(sw.sync_fresh_max[n_iters], h.fresh);
    }
    if (h.inside)
      for (int j = 0; j < h.fresh; ++j) {                            // every entry exactly once and in order
        CHECK(p.h_iter[(size_t)(h.off + j)] == dev.log[(size_t)(handed + j)]);
        sw.entries += 1;
      }
    handed += h.fresh;
    logged_read = p.n_logged;
    issued_at_read = p.issued_upto;
    CHECK(handed == logged_read);
  };

  bool extra = false;
  while (iters_issued < max_iter || !extra) {
    if (iters_issued >= max_iter) extra = true;
    enqueue();
    while (tk.outstanding() > lag) collect();
  }
  while (tk.outstanding() > 0) collect();
  CHECK(handed == (int)dev.log.size());
  CHECK(iters_issued == max_iter && uncollected == 0);
}

static Sweep check_lbfgs_log() {
  Sweep sw;
  for (int max_iter = 0; max_iter <= 12; ++max_iter) {
    const int n_eval = max_iter > 0 ? max_iter - 1 : 0;              // evaluations behind iterations
    for (int n_iters = 1; n_iters <= 6; ++n_iters)
      for (int lag = 0; lag <= 3; ++lag)
        for (unsigned pattern = 0; pattern < (1u << n_eval); ++pattern)
          for (int brk = 0; brk <= n_eval; ++brk) run_model(max_iter, n_iters, lag, pattern, brk, sw);
  }
  // the synchronous bound is tight: a call of n_iters iterations can hand out n_iters entries (and never more, above)
  for (int n_iters = 1; n_iters <= 6; ++n_iters) CHECK(sw.sync_fresh_max[n_iters] == n_iters);
  // a few windows by hand: fresh context, 3 iterations, room 13 -> 4; 5 issued since the last look -> 9; room left 2 -> 2
  CHECK(lbfgs_window(0, 0, 3, 13, 0, 12) == 4);
  CHECK(lbfgs_window(7, 2, 3, 13, 1, 12) == 9);
  CHECK(lbfgs_window(7, 2, 3, 13, 11, 12) == 2);
  CHECK(lbfgs_window(0, 0, 3, 0, 0, 0) == 0);
  // and hand-outs: 2 of a window of 4 already handed out by an earlier ticket, 2 fresh; one past the window is outside
  const LbfgsHandout a = lbfgs_handout(7, 5, 3, 4), b = lbfgs_handout(8, 5, 3, 4), c = lbfgs_handout(5, 5, 3, 4);
  CHECK(a.off == 2 && a.fresh == 2 && a.inside);
  CHECK(b.off == 2 && b.fresh == 3 && !b.inside);
  CHECK(c.off == 2 && c.fresh == 0 && c.inside);
  CHECK(!lbfgs_handout(4, 2, 3, 4).inside);                           // a window that starts behind what is due
  return sw;
}

int main() {
  check_tickets();
  check_adam();
  check_ring();
  const Sweep sw = check_lbfgs_log();
  if (g_failed) {
    fprintf(stderr, "optim_host_check: %ld checks failed\n", g_failed);
    return 1;
  }
  printf("optim_host_check ok: %ld runs, %ld collects, %ld entries handed out, least unclipped window slack %d\n", sw.runs,
         sw.collects, sw.entries, sw.slack_min);
  return 0;
}
