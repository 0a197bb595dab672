"""Host-only check that reserve_candidates() of gr_baz_amd/csrc/baz_music_hip.hip reserves what the commit before the scan-dispatch
refactor reserved (c187b3b: cand_entries / cand_entries_upto), for every context and batch of a grid: both versions of the arithmetic
are cut out of the two sources, compiled into one program under -fsanitize=address,undefined and compared.
usage: python scripts/cand_reservation_check.py [parent-commit = c187b3b]   (needs g++ and the git history)"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "gr_baz_amd/csrc/baz_music_hip.hip"


def cut(s, a, b):
    i = s.index(a)
    return s[i:s.index(b, i)]


PRE = '''#include <cstdint>
#include <cstddef>
#include <algorithm>
#include <cstdio>
struct Tab { const void* dCS; const void* dIB; };
struct baz_music_ctx { uint32_t m, n, fb_steps, nclass, num_cus, cs_tiles; int force_nsplit, coarse_rg; Tab tab; };
constexpr int cs_groups(int m) { return (m * m + 15) / 16; }
static uint32_t round_up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }
'''
MAIN = '''
int main() {
    static int dummy; unsigned long long cases = 0, bad = 0;
    const uint32_t ress[] = {1, 7, 63, 64, 65, 200, 256, 360, 361, 1000, 3600, 4096, 4097, 36000, 70000};
    const uint32_t batches[] = {1, 2, 15, 16, 17, 63, 64, 65, 100, 255, 256, 257, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193,
                                16384, 20000, 65536, 100000, 131072, 262144, 262145, 1000000, 4000000};
    const int forces[] = {0, 1, 2, 3, 8, 15, 16, 17, 63, 64, 65, 1000};
    const uint32_t cus[] = {1, 64, 256, 304};
    for (uint32_t m = 2; m <= 16; ++m) for (uint32_t n = 1; n < m; ++n) for (uint32_t res : ress) for (int f : forces) for (uint32_t cu : cus)
    for (int cs = 0; cs < 2; ++cs) for (int ib = 0; ib < 2; ++ib) for (int rg = 2; rg <= 4; rg += 2) for (uint32_t b : batches)
    for (uint32_t nc = 1; nc <= 4; nc *= 2) {
        baz_music_ctx c{m, n, (res + 63) / 64, nc, cu, round_up((res + 15) / 16, 8), f, rg, {cs ? &dummy : nullptr, ib ? &dummy : nullptr}};
        const size_t a = oldv::reserve(&c, b), z = newv::reserve(&c, b); ++cases;
        if (a != z && bad++ < 10) printf("DIFF m=%u n=%u res=%u force=%d cu=%u cs=%d ib=%d rg=%d batch=%u nclass=%u: %zu vs %zu\\n", m, n, res, f, cu, cs, ib, rg, b, nc, a, z);
    }
    printf("%llu cases, %llu differ\\n", cases, bad); return bad != 0;
}
'''


def main():
    commit = sys.argv[1] if len(sys.argv) > 1 else "c187b3b"
    new = open(os.path.join(ROOT, SRC)).read()
    old = subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (commit, SRC)]).decode()
    o = (cut(old, "struct ScanGeom {", "int ensure_candidates") + cut(old, "constexpr int coarse_rg_wide", "// ---- sorting in front") +
         cut(old, "uint32_t topn_list_len", "int reserve_candidates"))
    o += "size_t reserve(const baz_music_ctx* c, uint32_t batch) { return std::max(cand_entries(c, batch), cand_entries_upto(c, batch)); }\n"
    n = cut(new, "uint32_t topn_list_len", "int ensure_candidates") + cut(new, "constexpr int coarse_rg_wide", "// the candidate buffer for launches")
    n += ("size_t reserve(const baz_music_ctx* c, uint32_t batch) { const size_t ranges = std::max(scan_cand_ranges(c, batch), "
          "std::max(coarse_cand_ranges(c, batch), i8_cand_ranges(c, batch))); return ranges * topn_list_len(c->n); }\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "check.cpp"), "w").write(PRE + "namespace oldv {\n" + o + "}\nnamespace newv {\n" + n + "}\n" + MAIN)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-o", os.path.join(d, "check"), os.path.join(d, "check.cpp")])
        return subprocess.call([os.path.join(d, "check")])


if __name__ == "__main__":
    sys.exit(main())
