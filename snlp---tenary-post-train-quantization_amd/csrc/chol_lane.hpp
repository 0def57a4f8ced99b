// The straight-line step stream of chol.hip's one-lane-per-column panel solve and in-block
// triangular inverse: a constexpr schedule (plain C++17, a host compiler can include it) and the
// per-item device code expanded from it.
//
// A lane holds the 64 chains of one panel column (or one inverse row) as 32 register pairs.  The
// factored 64 x 64 diagonal block sits in LDS; its entries are wave-uniform, read as "items" --
// one ds_read_b128 of 4-group c of row R -- in a fixed stream with PRE items in flight (exact
// lgkmcnt waits, so register pressure stays at the chains plus PRE items instead of whatever the
// compiler would hoist).  Item (R, c) applies row R's terms to chains 4c .. 4c+3 (those > R).
//
// Stream order keeps every chain's terms in ascending row order (the PT2Q contract): row R's
// items follow all of row R-1's items, except the "diagonal item" of row R (its 4-group holding
// column R), which is read right after the row R-1 item holding column R -- by then chains of
// that group have every term of rows < R, chain R is final, and the division (panel: x_R / U_RR;
// inverse: (R == kl ? 1 : -x_R) / U_RR) overlaps the rest of row R-1's terms.
#pragma once

namespace pt2q_lane {

constexpr int NB = 64;                                 // block width (chol.hip's)
constexpr int PRE = 10;                                // items in flight
constexpr int N = (NB / 4) * (NB / 4 + 1) / 2 * 4;     // items (R, c) with c >= R / 4

struct Item {
  int R, c;
  bool diag;
};
struct Stream {
  Item it[N];
};

// Items in consumption order.
constexpr Stream make_stream() {
  Stream s{};
  int n = 0;
  s.it[n++] = {0, 0, true};
  for (int R = 0; R < NB; ++R)
    for (int c = R / 4; c < NB / 4; ++c) {
      if (c != R / 4) s.it[n++] = {R, c, false};  // (row R's diagonal item was placed during row R-1, or leads)
      if (R + 1 < NB && c == (R + 1) / 4) s.it[n++] = {R + 1, c, true};  // right after the row-R item holding column R+1
    }
  return s;
}
constexpr Stream STREAM = make_stream();

constexpr Item item(int i) { return STREAM.it[i]; }
constexpr int offset(int i) { return (item(i).R * NB + 4 * item(i).c) * 4; }  // LDS bytes of U[R][4c]
constexpr int slot(int i) { return i % PRE; }
constexpr int issued(int i) { return i + PRE < N ? i + PRE : N; }  // reads issued when item i is waited for
constexpr int wait(int i) { return issued(i) - i - 1; }            // ... of which these follow item i
// Item i writes chain pair p (chains 2p, 2p + 1): its division, or a term of row R.  The next
// item's wait ties those pairs into its operands, so the compiler keeps each item's FMAs between
// its wait and the next one's.
constexpr bool writes(int i, int p) {
  return (item(i).diag && p == item(i).R / 2) || (p / 2 == item(i).c && 2 * p + 1 > item(i).R);
}

// Each (R, c >= R / 4) once; row R's diagonal item comes when chain R has exactly rows 0 .. R-1
// and before any other item of row R; every term a chain receives is its next row in order.
constexpr bool chain_order_ok() {
  int terms[NB] = {};  // chain j has received rows 0 .. terms[j] - 1
  bool fin[NB] = {}, seen[NB][NB / 4] = {};
  for (int i = 0; i < N; ++i) {
    const Item a = item(i);
    if (a.c < a.R / 4 || a.c >= NB / 4 || seen[a.R][a.c]) return false;
    seen[a.R][a.c] = true;
    if (a.diag) {
      if (a.c != a.R / 4 || terms[a.R] != a.R) return false;
      fin[a.R] = true;
    }
    if (!fin[a.R]) return false;
    for (int j = 4 * a.c; j < 4 * a.c + 4; ++j)
      if (j > a.R && terms[j]++ != a.R) return false;
  }
  for (int j = 0; j < NB; ++j)
    if (terms[j] != j || !fin[j]) return false;
  return true;
}
static_assert(chain_order_ok(), "lane stream: every chain takes rows 0 .. j-1 in ascending order");

// LDS returns a wave's reads in order, so at item i's wait the first issued(i) - wait(i) reads
// have landed: item i must be among them and still own its slot, and the read issued after item
// i's uses (item i + PRE) must go into a slot whose item is consumed.
constexpr bool ring_ok() {
  int owner[PRE] = {};
  for (int i = 0; i < PRE; ++i) owner[slot(i)] = i;
  for (int i = 0; i < N; ++i) {
    if (wait(i) < 0 || issued(i) - wait(i) <= i || owner[slot(i)] != i) return false;
    if (i + PRE < N) {
      if (owner[slot(i + PRE)] > i) return false;
      owner[slot(i + PRE)] = i + PRE;
    }
  }
  return true;
}
static_assert(ring_ok(), "lane stream: waits cover their item, no slot re-issued before its use");

#ifdef PT2Q_DEV  // device code: chol.hip includes this after common.hpp, its f32x2 / f32x4 and NB
static_assert(NB == pt2q_chol::NB, "the stream is written for chol.hip's block width");

template <int I>
PT2Q_DEV void issue(f32x4 (&t)[PRE], uint32_t ds) {
  if constexpr (I < N)
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(t[slot(I)]) : "v"(ds), "n"(offset(I)));
}

// Row R's terms for chain pair P out of the item d (chain 2P takes none when 2P <= R).
template <int R, int P>
PT2Q_DEV void terms(f32x2 (&xp)[NB / 2], const f32x2 (&b)[NB], f32x4 d) {
  constexpr int h = P % 2;
  if constexpr (2 * P > R)
    xp[P] = __builtin_elementwise_fma(__builtin_shufflevector(d, d, 2 * h, 2 * h + 1), b[R], xp[P]);
  else if constexpr (2 * P + 1 > R)
    xp[P][1] = fmaf(d[2 * h + 1], b[R][0], xp[P][1]);
}

template <bool INV, int I>
PT2Q_DEV void step(f32x2 (&xp)[NB / 2], f32x2 (&b)[NB], f32x4 (&t)[PRE], uint32_t ds, int kl) {
  constexpr int R = item(I).R, c = item(I).c, s = slot(I);
  constexpr int q = I > 0 ? 2 * item(I > 0 ? I - 1 : 0).c : 0;  // the previous item's pairs q, q + 1
  constexpr bool lo = I > 0 && writes(I - 1, q), hi = I > 0 && writes(I - 1, q + 1);
  static_assert(hi || !lo, "an item that writes its low pair writes the high one too");
  if constexpr (lo)
    asm volatile("s_waitcnt lgkmcnt(%[w])" : "+v"(t[s]), "+v"(xp[q]), "+v"(xp[q + 1]) : [w] "n"(wait(I)));
  else if constexpr (hi)
    asm volatile("s_waitcnt lgkmcnt(%[w])" : "+v"(t[s]), "+v"(xp[q + 1]) : [w] "n"(wait(I)));
  else
    asm volatile("s_waitcnt lgkmcnt(%[w])" : "+v"(t[s]) : [w] "n"(wait(I)));
  if constexpr (item(I).diag) {
    if constexpr (INV)
      xp[R / 2][R % 2] = (R == kl ? 1.0f : -xp[R / 2][R % 2]) / t[s][R % 4];
    else
      xp[R / 2][R % 2] = xp[R / 2][R % 2] / t[s][R % 4];
    if constexpr (R + 1 < NB) {  // the last row has no terms to apply
      if constexpr (INV)
        b[R] = f32x2{xp[R / 2][R % 2], xp[R / 2][R % 2]};
      else
        b[R] = f32x2{-xp[R / 2][R % 2], -xp[R / 2][R % 2]};  // (-U)·x == U·(-x)
    }
  }
  terms<R, 2 * c>(xp, b, t[s]);
  terms<R, 2 * c + 1>(xp, b, t[s]);
  issue<I + PRE>(t, ds);
}

// The stream is expanded in runs of RUN items: one fold over all N nests deeper than clang allows.
constexpr int RUN = 32;
static_assert(N % RUN == 0, "whole runs");

template <bool INV, int I0, int... K>
PT2Q_DEV void run(f32x2 (&xp)[NB / 2], f32x2 (&b)[NB], f32x4 (&t)[PRE], uint32_t ds, int kl,
                  std::integer_sequence<int, K...>) {
  (step<INV, I0 + K>(xp, b, t, ds, kl), ...);
}

template <bool INV, int... P, int... J>
PT2Q_DEV void runs(f32x2 (&xp)[NB / 2], uint32_t ds, int kl, std::integer_sequence<int, P...>,
                   std::integer_sequence<int, J...>) {
  f32x4 t[PRE];
  f32x2 b[NB];  // b[R]: row R's final value in both halves (negated in the panel solve)
  (issue<P>(t, ds), ...);
  (run<INV, RUN * J>(xp, b, t, ds, kl, std::make_integer_sequence<int, RUN>{}), ...);
}

// xp: the lane's chains; ds: LDS address of the staged block; kl: the inverse row's own diagonal
// step (unused in the panel solve).
template <bool INV>
PT2Q_DEV void stream(f32x2 (&xp)[NB / 2], uint32_t ds, int kl) {
  runs<INV>(xp, ds, kl, std::make_integer_sequence<int, PRE>{}, std::make_integer_sequence<int, N / RUN>{});
}
#endif  // PT2Q_DEV

}  // namespace pt2q_lane
