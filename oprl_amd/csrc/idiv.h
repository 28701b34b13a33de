// idiv.h — index divisions by a divisor that is the same for every thread, every launch and the whole life of a learner
// (state size, action size, tiles per row of a layer), without the divide.
//
// hipcc expands `n / d` with a run-time d into ~30 instructions (reciprocal, two corrections), in every wave that
// meets it; the chain launch's role prologues, its critic pass and its tiles meet such a division a dozen times
// per update.  Two replacements, both EXACT on their stated domain — the quotient is an index: it changes which
// address a thread computes, never an operand — and both checked exhaustively on the host (tests/host/idiv_check.cpp):
//   row_div    n / d through a multiplier the HOST forms once (ChainArgs::mS / mA / mSA): one multiply and one shift
//   small_div  n / d for d <= 8 (columns of a narrow tile, 64-column blocks of a layer's fan-in) from a table packed
//              into two constants: no argument to carry, no branch
// Needs no device: plain C++ for the host check, __host__ __device__ under hipcc.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OPRL_HD __host__ __device__
#else
#define OPRL_HD
#endif

namespace oprl {

// ---- row_div: 0 <= n < kRowDivMaxN, 1 <= d <= kRowDivMaxD.
// m = floor(2^20 / d) + 1, so m d = 2^20 + e with 1 <= e <= d, and n m / 2^20 = n / d + n e / (d 2^20): the floor is
// that of n / d as long as n e < 2^20, which n d < 2^20 guarantees; n m <= n 2^20 / d + n stays below 2^32.
constexpr int kRowDivShift = 20;
constexpr int kRowDivMaxN = 4096;      // kR rows x (at most 256 columns)
constexpr int kRowDivMaxD = 256;
OPRL_HD inline unsigned row_div_magic(int d) { return (1u << kRowDivShift) / (unsigned)d + 1u; }
OPRL_HD inline bool row_div_ok(int d) { return d >= 1 && d <= kRowDivMaxD; }
OPRL_HD inline int row_div(int n, unsigned m) { return (int)(((unsigned)n * m) >> kRowDivShift); }

// ---- small_div: 0 <= n < kSmallDivMaxN, 1 <= d <= kSmallDivMaxD — the CALLER's shapes guarantee both (no fall-back: a
// branch to a division that is never taken still costs its test and the division's code in every wave): a narrow tile
// has at most 8 valid columns and 128 elements (tp4.h), a layer of the lean shapes — width 256, fan-in <= 96: what every
// launcher of the 16 x 64 tiles asks for (fused_ddpg.hip lean_ok) — at most four 64-column blocks and 192 tiles.
// Beyond the domain the quotient is WRONG without a diagnostic, so the launchers of the code that calls this say the
// limits themselves, on the host, before they launch: fused_ddpg.hip narrow8_ok / tiles64_ok and the static_asserts there.
// ceil(2^15 / d) for d = 1 .. 8, 16 bits each: m d - 2^15 <= 6, so the quotient is exact for n < 2^15 / 6.
constexpr int kSmallDivMaxN = 5461, kSmallDivMaxD = 8;
constexpr unsigned long long kSmallDivLo = 32768ull | (16384ull << 16) | (10923ull << 32) | (8192ull << 48);     // d = 1 .. 4
constexpr unsigned long long kSmallDivHi = 6554ull | (5462ull << 16) | (4682ull << 32) | (4096ull << 48);        // d = 5 .. 8
OPRL_HD inline int small_div(int n, int d) {
  const unsigned m = (unsigned)((d > 4 ? kSmallDivHi : kSmallDivLo) >> (((d - 1) & 3) * 16)) & 0xffffu;
  return (int)(((unsigned)n * m) >> 15);
}

}  // namespace oprl
