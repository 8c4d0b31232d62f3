// optim_host.h -- what the optimiser drivers of engine.hip decide on the host without a device, stated once: the counters of
// the chunks in flight, Adam's bias-corrected step factors, the layout of Adam's loss ring, and the window of L-BFGS log
// entries a chunk copies and hands out.  Plain C++: no HIP include and no kernel code, so a host compiler alone builds it
// (tests/host/optim_host_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>

namespace pinn {

// chunks of optimiser steps the host has not collected yet (pinn_ctx::Pending): at most this many at a time
constexpr int N_PENDING = 4;

// Tickets: chunk i of a context's lifetime goes into slot i % N_PENDING and carries the number i mod 2^31 (an int the C API
// hands out); chunks are collected in the order they were issued.
struct Tickets {
  unsigned long long issued = 0, collected = 0;
  int outstanding() const { return (int)(issued - collected); }
  bool room() const { return outstanding() < N_PENDING; }
  int next_slot() const { return (int)(issued % N_PENDING); }         // where the next ticket's chunk goes
  int next_number() const { return (int)(issued & 0x7fffffff); }
  int oldest_slot() const { return (int)(collected % N_PENDING); }
  bool is_oldest(int ticket) const { return outstanding() > 0 && ticket == (int)(collected & 0x7fffffff); }
  void drop_all() { collected = issued; }                             // a restart: results in flight are forgotten
};

// Adam's bias correction at step t >= 1: a step of rate lr is lr sqrt(1 - b2^t) / (1 - b1^t).  The operation order is part of
// the contract -- (lr * s) / d, not lr * (s / d): an ensemble member is bit-identical to a context of its own only while
// every step size is formed this way.
struct AdamFactors {
  double s, d;
  AdamFactors(double b1, double b2, double t) : s(std::sqrt(1.0 - std::pow(b2, t))), d(1.0 - std::pow(b1, t)) {}
  double alpha(double lr) const { return lr * s / d; }
  double bc_pw() const { return s / d; }                              // the correction alone (adr point weights: rates on the device)
};

// Adam's loss ring on the device: N_PENDING regions (one per chunk in flight) of `stride` steps x 3 loss parts.
inline size_t ring_steps(int n_steps) { return n_steps < 16 ? 16 : (size_t)n_steps; }    // at least 16 steps per region
inline size_t ring_doubles(size_t steps) { return steps * N_PENDING * 3; }
inline bool ring_must_grow(size_t steps, size_t capacity_bytes) { return ring_doubles(steps) * 8 > capacity_bytes; }
inline size_t ring_region(const Tickets& tk, size_t stride) { return (size_t)tk.next_slot() * stride * 3; }   // next ticket's

// The L-BFGS log.  The device appends one (nIter, f) entry per evaluation that passes every break test; the host has handed
// out the first logged_read of them, a figure it brought up to date when iters_issued stood at issued_at_read.
// lbfgs_window: the entries a chunk of n_iters iterations copies to its pinned buffers, counted from entry logged_read: one
// per evaluation settled since the host last looked -- the iterations issued since then, this chunk's, + 1 -- clipped to
// the log's room.
inline int lbfgs_window(int iters_issued, int issued_at_read, int n_iters, int log_room, int logged_read, int max_iter) {
  int window = (iters_issued - issued_at_read) + n_iters + 1;
  if (window > log_room - logged_read) window = log_room - logged_read;
  if (window < 0 || max_iter == 0) window = 0;
  return window;
}

// lbfgs_handout: at collect the chunk's state says n_logged; the host has handed out logged_read by now (an earlier ticket
// may have moved it since the chunk was issued, when it stood at base).  Entries off .. off + fresh - 1 of the chunk's window
// are due; inside = they all lie in the window that was copied.
struct LbfgsHandout { int off, fresh; bool inside; };
inline LbfgsHandout lbfgs_handout(int n_logged, int logged_read, int base, int window) {
  const int fresh = n_logged > logged_read ? n_logged - logged_read : 0;
  const int off = logged_read - base;
  return {off, fresh, off >= 0 && off + fresh <= window};
}

}  // namespace pinn
