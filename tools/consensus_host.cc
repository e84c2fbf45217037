// The consensus selection of include/slimt_hip.h (slimt_hip_consensus_select) as a host loop: what a caller without the
// device selection runs after a fan-out call has returned its rows. tools/consensus_bench.py builds this file into a shared
// library and times it beside the armed call; it is also a second host statement of the definition (sorted multisets merged
// pairwise), bit for bit the device's result.
//   g++ -O2 -std=c++17 -fPIC -shared tools/consensus_host.cc -o consensus_host.so
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {
using Gram = std::array<uint32_t, 4>;  // a g-gram, zero behind its g tokens

// the sorted g-grams of one row
std::vector<Gram> grams(const uint32_t *row, int n, int g) {
  std::vector<Gram> out;
  for (int p = 0; p + g <= n; ++p) {
    Gram x{};
    for (int i = 0; i < g; ++i) x[(size_t)i] = row[p + i];
    out.push_back(x);
  }
  std::sort(out.begin(), out.end());
  return out;
}

// the clipped match count of two sorted multisets
int matches(const std::vector<Gram> &a, const std::vector<Gram> &b) {
  size_t i = 0, j = 0;
  int m = 0;
  while (i < a.size() && j < b.size()) {
    if (a[i] < b[j]) {
      ++i;
    } else if (b[j] < a[i]) {
      ++j;
    } else {
      ++m;
      ++i;
      ++j;
    }
  }
  return m;
}
}  // namespace

extern "C" int consensus_host(const uint32_t *ids, const uint32_t *len, const uint32_t *row_src, size_t N, size_t T, size_t B,
                              int max_order, int beta2, double *utility, uint32_t *best) {
  if (max_order < 1 || max_order > 4 || beta2 < 1 || beta2 > 16 || B == 0 || T == 0) return -1;
  std::vector<std::vector<uint32_t>> rows_of(B);
  for (size_t c = 0; c < N; ++c) {
    if (row_src[c] >= B || len[c] > T) return -1;
    utility[c] = 0.0;
    if (len[c] > 0) rows_of[row_src[c]].push_back((uint32_t)c);  // (ascending; competing rows only)
  }
  for (size_t b = 0; b < B; ++b) {
    const std::vector<uint32_t> &rows = rows_of[b];
    const size_t n = rows.size();
    best[b] = 0xFFFFFFFFu;
    if (n == 0) continue;
    std::vector<std::vector<Gram>> g_of(n * 4);
    for (size_t x = 0; x < n; ++x)
      for (int g = 1; g <= max_order; ++g) g_of[x * 4 + (size_t)(g - 1)] = grams(ids + (size_t)rows[x] * T, (int)len[rows[x]], g);
    std::vector<int> M(n * n * 4, 0);
    for (size_t h = 0; h < n; ++h)
      for (size_t r = h + 1; r < n; ++r)
        for (int g = 0; g < max_order; ++g)
          M[(h * n + r) * 4 + (size_t)g] = M[(r * n + h) * 4 + (size_t)g] = matches(g_of[h * 4 + (size_t)g], g_of[r * 4 + (size_t)g]);
    double top = 0.0;
    for (size_t h = 0; h < n; ++h) {
      const int nh = (int)len[rows[h]];
      double sum = 0.0;
      int refs = 0;
      for (size_t r = 0; r < n; ++r) {
        if (r == h) continue;
        const int nr = (int)len[rows[r]];
        double us = 0.0;
        int counted = 0;
        for (int g = 1; g <= max_order; ++g) {
          const int ch = std::max(nh - g + 1, 0), cr = std::max(nr - g + 1, 0);
          if (ch == 0 && cr == 0) continue;
          us = us + (double)((1 + beta2) * M[(h * n + r) * 4 + (size_t)(g - 1)]) / (double)(beta2 * cr + ch);
          ++counted;
        }
        sum = sum + (counted ? us / (double)counted : 0.0);
        ++refs;
      }
      const double u = refs ? sum / (double)refs : 0.0;
      utility[rows[h]] = u;
      if (best[b] == 0xFFFFFFFFu || u > top) {
        best[b] = rows[h];
        top = u;
      }
    }
  }
  return 0;
}
