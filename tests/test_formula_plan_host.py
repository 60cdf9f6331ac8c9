"""The lookup facts of a boolean-rewrite plan (fplan_lookup_facts, keto_amd/csrc/kg_formula.h) on the host,
no GPU: lookup_ok = !f(0), and the walk leaves J of the rule "from the highest leaf index down, drop a leaf if f
stays false under every assignment of the dropped leaves while the kept ones are false".  A small program
includes the header, builds the postfix plans by hand and prints both facts; it also checks, for every plan
with lookup_ok, what the lookups rely on: f is false under every assignment whose J leaves are all false."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "kg_formula.h"
using namespace kg;
static int facts(uint32_t n_leaves, std::initializer_list<int> ops) {
  FPlan P{};
  P.n_leaves = n_leaves;
  for (int op : ops) P.ops[P.n_ops++] = (uint8_t)op;
  fplan_lookup_facts(P);
  std::printf("%u %u\n", P.lookup_ok, P.walk_leaves);
  if (!P.lookup_ok) return P.walk_leaves != 0;
  for (uint32_t a = 0; a < (1u << n_leaves); a++)
    if (!(a & P.walk_leaves) && fplan_eval(P, a)) return 1;  // a member no walk leaf knows
  return 0;
}
int main() {
  const int L = FOP_LEAF, NOT = FOP_NOT, AND = FOP_AND, OR = FOP_OR;
  int bad = 0;
  bad |= facts(2, {L | 0, L | 1, NOT, AND | 2});                           // and(u, not blocked)
  bad |= facts(3, {L | 0, L | 1, NOT, AND | 2, L | 2, OR | 2});            // or(and(u2, not a), blocked)
  bad |= facts(2, {L | 0, L | 1, AND | 2});                                // and(a, b)
  bad |= facts(1, {L | 0, NOT, OR | 1});                                   // not u1
  bad |= facts(3, {L | 0, L | 1, AND | 2, NOT, L | 2, NOT, AND | 2});      // not(and(a, b)) & not u2
  bad |= facts(2, {L | 0, L | 1, OR | 2});                                 // or(a, b)
  bad |= facts(4, {L | 0, L | 1, OR | 2, L | 2, L | 3, OR | 2, AND | 2});  // and(or(a, b), or(c, d))
  bad |= facts(2, {L | 0, L | 1, NOT, OR | 2, L | 0, AND | 2});            // and(or(a, not b), a)
  return bad;
}
"""

# lookup_ok, walk leaves as a bit mask
WANT = [(1, 0b01), (1, 0b101), (1, 0b01), (0, 0), (0, 0), (1, 0b11), (1, 0b0011), (1, 0b01)]


def test_plan_lookup_facts(tmp_path):
    from keto_amd import build
    src, exe = tmp_path / "facts.hip", tmp_path / "facts"
    src.write_text(PROGRAM)
    subprocess.run([build.HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I",
                    os.path.join(ROOT, "keto_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert got == WANT, got
    assert r.returncode == 0  # f is false wherever every walk leaf is
