// Host-only check of csrc/idiv.h: the divide-free index arithmetic of the chain launch against the plain division,
// over every divisor and every dividend the kernels can meet.  Stand-alone (its own main), built with
// -fsanitize=address,undefined by tests/test_idiv_host.py; exit status 0 = every quotient exact and the sanitizers quiet.
#include <cstdio>
#include <vector>

#include "../../oprl_amd/csrc/idiv.h"

using namespace oprl;

namespace {
constexpr int kR = 16;             // rows of a slice (engine.h)
constexpr int kThreads = 1024;     // threads of a workgroup
int fails = 0;

void expect(bool ok, const char* what, long a, long b, long c) {
  if (!ok && fails++ < 20) std::fprintf(stderr, "FAIL %s: %ld %ld %ld\n", what, a, b, c);
}

// the row / column split as the kernels spell it: row = idx / k, col = idx - row * k
void check_rows(int k, int n_idx) {
  const unsigned m = row_div_magic(k);
  for (int idx = 0; idx < n_idx; ++idx) {
    const int row = row_div(idx, m);
    expect(row == idx / k, "row_div", idx, k, row);
    expect(idx - row * k == idx % k, "row_div column", idx, k, row);
  }
}
}  // namespace

int main() {
  // ---- the whole stated domain of row_div
  for (int d = 1; d <= kRowDivMaxD; ++d) {
    expect(row_div_ok(d), "row_div_ok", d, 0, 0);
    check_rows(d, kRowDivMaxN);
    std::printf("magic %d %u\n", d, row_div_magic(d));
  }
  expect(!row_div_ok(0) && !row_div_ok(kRowDivMaxD + 1), "row_div_ok bounds", 0, 0, 0);
  // ---- the shapes a learner can have (state sizes 1 .. 90, action sizes 1 .. 21 within the layer-0 fan-in limit of 96),
  // over the indices the kernel forms: the roles' loops run idx < kR * k; the critic pass's prologue takes tid and
  // tid + kThreads whatever S is
  std::vector<int> seen(kRowDivMaxD + 1, 0);
  for (int S = 1; S <= 90; ++S)
    for (int A = 1; A <= 21; ++A) {
      if (S + A > 96) continue;
      for (int k : {S, A, S + A}) {
        expect(row_div_ok(k), "shape divisor", S, A, k);
        if (seen[k]++) continue;
        check_rows(k, kR * k);
        check_rows(k, 2 * kThreads);
      }
    }
  // ---- small_div: every divisor over its stated domain
  for (int d = 1; d <= kSmallDivMaxD; ++d)
    for (int n = 0; n < kSmallDivMaxN; ++n) expect(small_div(n, d) == n / d, "small_div", n, d, small_div(n, d));
  // the narrow exchange's element split (tp4.h: 64 lanes x 2 slots over a 16 x ncols block)
  for (int ncols = 1; ncols <= 8; ++ncols)
    for (int e = 0; e < 16 * ncols; ++e) {
      const int row = small_div(e, ncols);
      expect(row == e / ncols && e - row * ncols == e % ncols && row < 16, "narrow element", e, ncols, row);
    }
  // the tile coordinates (dw_tile_x2.h: tn = lt / tiles_k with tiles_k 64-column blocks of the fan-in — 256 at most in the
  // lean shapes, swept to 512 — and at most 192 tiles per net in a chain launch)
  for (int K = 1; K <= 512; ++K) {
    const int tiles_k = (K + 63) / 64;
    for (int lt = 0; lt < 192 * 4; ++lt) {
      const int tn = small_div(lt, tiles_k);
      expect(tn == lt / tiles_k && lt - tn * tiles_k == lt % tiles_k, "tile coordinates", lt, K, tn);
    }
  }
  if (fails) { std::fprintf(stderr, "%d mismatches\n", fails); return 1; }
  std::puts("idiv_check: ok");
  return 0;
}
