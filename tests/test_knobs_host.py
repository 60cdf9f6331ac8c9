"""The knob table (keto_amd/csrc/kg_knobs.h) against a list of its own: every kg_snapshot_tune key with the field
it stores to, its default and its accepted range, as the library had them before the table existed (one strcmp
stanza per key, one field of the snapshot each).  A stand-alone C++ program written from that list names every
field and checks defaults, both bounds, the values just outside them and that a store touches one field only;
it needs no GPU and no HIP.  Also built under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_BOUND = (1 << 63) - 1  # "no upper bound": every int64 value from lo on

# (key, field, default, lo, hi)
KNOBS = [
    ("shard_vis", "shard_vis_log2", 23, 10, 34),
    ("shard_bucket", "shard_bucket0", 0, 0, 1 << 26),
    ("shard_force_exchange", "shard_force_exchange", 0, 0, 1),
    ("shard_local", "shard_local", 1, 0, 1),
    ("shard_remote_meta", "shard_remote_meta", 1, 0, 1),
    ("shard_max_reruns", "shard_max_reruns", 0, 0, 64),
    ("shard_max_bytes", "shard_max_bytes", 0, 0, NO_BOUND),
    ("shard_force_overflow", "shard_force_overflow", 0, 0, 1),
    ("stream_ecap", "stream_ecap", 512, 0, 0xFFFFFFFF),
    ("shard_budget", "shard_budget", 0, 0, 0xFFFFFFFF),
    ("shard_heavy", "shard_heavy", 64, 0, 0xFFFFFFFF),
    ("shard_back_budget", "shard_back_budget", 1 << 14, 0, 0xFFFFFFFF),
    ("holder_sig", "holder_sig", 1, 0, 1),
    ("stream_steal", "stream_steal", 4, 1, 8),
    ("stream_wgs", "stream_wgs", 2, 0, 8),
    ("grid_wgs", "grid_wgs", 2, 1, 64),
    ("interp_cap2", "interp_cap2", 0, 0, 1 << 22),
    ("grid_cap", "grid_small_cap", 0, 0, 1 << 34),
    ("expand_gw", "expand_gw", 1, 0, 1),
    ("expand_skip_lds", "expand_skip_lds", 0, 0, 2),
    ("expand_hash_cap", "expand_hash_cap", 1 << 18, 4, 1 << 18),
    ("level_events", "level_events", 0, 0, 1),
    ("expand_gw_wait_us", "expand_gw_wait_us", 100000, 0, 10000000),
    ("grid_ms", "grid_ms", 1, 0, 1),
    ("grid_ms_bytes", "grid_ms_bytes", 1 << 30, 1 << 20, 1 << 40),
    ("grid_ms_words", "grid_ms_words", 8, 1, 16),  # and a power of two
    ("grid_ms_tg_cap", "grid_ms_tg_cap", 256, 0, 0x7FFFFFFF),
    ("grid_ms_cap", "grid_ms_cap", 0, 0, 1 << 28),
    ("max_lanes", "lane_cap", 32, 1, 1024),
    ("lookup_cap", "lookup_cap", 0, 0, 1 << 32),
    ("lookup_domain_rows", "lookup_domain_rows", 0, 0, 1),
    ("lookup_formula", "lookup_formula", 1, 0, 1),
    ("query_cap", "query_cap", 0, 0, 1 << 32),
    ("back_edges", "back_edges", 0, 0, 1 << 20),
    ("back_wgs", "back_wgs", 3, 1, 3),
]
# values inside a key's range that it refuses all the same
HOLES = {"grid_ms_words": [3, 5, 6, 7, 12, 15]}
# keys that kg_snapshot_tune takes but the table does not hold (an action, nothing stored), and ones nobody takes
NOT_IN_TABLE = ["grid_reserve", "no_such_knob", "shard_wgs", "interp_wgs", "lane_cap", "shard_vis_log2", ""]


def program() -> str:
    def lit(v):
        return f"{v}LL" if v > -(1 << 63) else "(-9223372036854775807LL - 1)"
    out = ['#include <cstdio>', '#include "kg_knobs.h"', 'using kg::Knobs;', 'static int bad = 0;',
           '#define EXPECT(c, ...) do { if (!(c)) { bad++; printf("FAIL %s:", #c); printf(__VA_ARGS__); printf("\\n"); } } while (0)',
           '// every field holds its default, but field `at` (an index of the list; -1: none), which holds v',
           'static void only(const Knobs& k, int at, long long v, const char* what) {']
    for i, (key, field, default, lo, hi) in enumerate(KNOBS):
        out.append(f'  EXPECT((long long)k.{field} == (at == {i} ? v : {lit(default)}), " {field} after %s", what);')
    out += ['}',
            'static void accepted(const char* key, int at, long long v) {',
            '  Knobs k;', '  const kg::Knob* row = nullptr;',
            '  EXPECT(kg::knob_set(k, key, v, &row) == 0, " %s = %lld", key, v);',
            '  EXPECT(row && strcmp(row->key, key) == 0, " row of %s", key);',
            '  only(k, at, v, key);', '}',
            'static void refused(const char* key, long long v) {',
            '  Knobs k;', '  const kg::Knob* row = nullptr;',
            '  EXPECT(kg::knob_set(k, key, v, &row) == kg::KNOB_OUT_OF_RANGE, " %s = %lld", key, v);',
            '  EXPECT(row && strcmp(row->key, key) == 0, " row of %s", key);',
            '  only(k, -1, 0, key);', '}',
            'int main() {',
            f'  EXPECT(kg::N_KNOBS == {len(KNOBS)}, " %zu keys in the header", (size_t)kg::N_KNOBS);',
            '  { Knobs k; only(k, -1, 0, "construction"); }']
    for i, (key, field, default, lo, hi) in enumerate(KNOBS):
        out += [f'  accepted("{key}", {i}, {lit(lo)});', f'  accepted("{key}", {i}, {lit(hi)});',
                f'  accepted("{key}", {i}, {lit(default)});']
        out.append(f'  refused("{key}", {lit(lo - 1)});')
        if hi != NO_BOUND:
            out.append(f'  refused("{key}", {lit(hi + 1)});')
        out.append(f'  refused("{key}", {lit(-(1 << 63))});')
        for v in HOLES.get(key, []):
            out.append(f'  refused("{key}", {lit(v)});')
    out.append('  refused("grid_ms_words", 32LL);')
    for v in (1, 2, 4, 8, 16):
        out.append(f'  accepted("grid_ms_words", {[k[0] for k in KNOBS].index("grid_ms_words")}, {v}LL);')
    for key in NOT_IN_TABLE:
        out += ['  {', '    Knobs k;', '    const kg::Knob* row = &kg::KNOBS[0];',
                f'    EXPECT(kg::knob_set(k, "{key}", 1, &row) == kg::KNOB_UNKNOWN, " unknown key {key}");',
                f'    EXPECT(row == nullptr, " no row for {key}");', f'    only(k, -1, 0, "unknown key {key}");', '  }']
    out += ['  if (!bad) printf("knobs ok\\n");', '  return bad ? 1 : 0;', '}', '']
    return "\n".join(out)


def test_the_list_is_a_list_of_distinct_keys_and_fields():
    assert len({k[0] for k in KNOBS}) == len(KNOBS) == len({k[1] for k in KNOBS})
    for key, field, default, lo, hi in KNOBS:
        assert lo <= default <= hi, key


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_knob_table_matches_the_list(tmp_path, sanitize):
    """The header alone, compiled by g++ into a program with its own main (nothing preloaded, no GPU used)."""
    if sanitize:
        import torch
        if torch.cuda.is_available():
            pytest.skip("sanitizer runs stay off GPU machines")
    src, exe = tmp_path / "knobs_check.cpp", tmp_path / "knobs_check"
    src.write_text(program())
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "keto_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "knobs ok" in r.stdout
