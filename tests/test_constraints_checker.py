"""slimt_amd/csrc/constraints.h (cn_greedy_row, built from the functions the kernel calls) as a stand-alone host program against
tests/support/constraints_ref.py: banned, seen and candidate sets, greedy column and fallback, exactly, on the GPU test's rows."""
import os
import subprocess

import numpy as np
import pytest

from support import constraints_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROGRAM = r"""
#include <stdio.h>
#include <vector>
#include "constraints.h"
using namespace slimt_hip;
// stdin: rows of "N L n theta-bits min_length eos n_suppress has_ids", N logit bit patterns, then the history, the suppress
// list and the ids in decimal; stdout per row: "banned... | seen... | candidates... | column lifted"
int main() {
  unsigned N, L, tb, eos, has;
  StepConstraints c;
  while (scanf("%u %u %u %x %u %u %u %u", &N, &L, &c.no_repeat_ngram, &tb, &c.min_length, &eos, &c.n_suppress, &has) == 8) {
    std::vector<float> l(N), z(N);
    std::vector<unsigned> h(L), sup(c.n_suppress), ids(has ? N : 0);
    std::vector<unsigned char> ban(N), seen(N);
    for (float &v : l) { unsigned b; if (scanf("%x", &b) != 1) return 1; v = sm_float(b); }
    for (auto *a : {&h, &sup, &ids}) for (unsigned &v : *a) if (scanf("%u", &v) != 1) return 1;
    c.theta = sm_float(tb);
    c.inv_theta = 1.0f / c.theta;
    if (!cn_valid(c.no_repeat_ngram, c.theta, c.n_suppress)) return 2;
    for (unsigned i = 0; i < c.n_suppress; ++i) c.suppress[i] = sup[i];
    bool lift;
    const int col = cn_greedy_row(l.data(), (int)N, has ? ids.data() : nullptr, h.data(), L, c, eos, ban.data(), seen.data(), z.data(), &lift);
    for (int set = 0; set < 3; ++set, printf(" |"))
      for (unsigned i = 0; i < N; ++i) if (set == 0 ? ban[i] : set == 1 ? seen[i] : cn_candidate(z[i], ban[i], lift)) printf(" %u", i);
    printf(" %d %d\n", col, (int)lift);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("constraints")
    (d / "main.cc").write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "slimt_amd", "csrc"),
                           str(d / "main.cc"), "-o", str(d / "constraints")])
    return str(d / "constraints")


@pytest.mark.parametrize("with_ids", [False, True])
def test_the_header_and_the_restatement_agree_on_the_crafted_rows(program, with_ids):
    cases = []
    for N in (1, 2, 63, 65, 4097):
        ids, eos = constraints_ref.layout(N, with_ids)
        cases += [(ids, eos) + row for row in constraints_ref.crafted_rows(N, ids, eos, 11 * N)]
    words = lambda a: " ".join(str(int(v)) for v in a)
    text = "".join("%d %d %d %x %d %d %d %d\n%s\n%s\n%s\n%s\n" % (
        x.size, len(h), cn[0], np.float32(cn[1]).view(np.uint32), cn[2], eos, len(cn[3]), ids is not None,
        " ".join("%x" % b for b in x.view(np.uint32)), words(h), words(cn[3]), words(ids if ids is not None else []))
        for ids, eos, _, x, h, cn in cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (ids, eos, kind, x, h, cn) in zip(out, cases, strict=True):
        got = [[int(v) for v in part.split()] for part in line.split("|")]
        grams, other, seen = constraints_ref.sets(h, cn, x.size, ids, eos)
        col, none, _, fallback, _, C, _ = constraints_ref.constrained_row(x, h, cn, ids, eos)
        assert got[:3] == [list(np.flatnonzero(s)) for s in (grams | other, seen, C)] and got[3][1] == fallback, (kind, x.size, with_ids)
        assert none or got[3][0] == col, (kind, x.size, with_ids)  # (none: "logit 0 is NaN", the record step's rule, not the row's)
