"""The hand-over schedule of the pipelined attention loop (ipdm-pytorch_amd/csrc/attn_pipe_schedule.h), replayed on the host: a
stand-alone program includes the header -- the functions the kernel's two sides index the LDS ring with -- and walks both sides
barrier by barrier for it0 in {0, 1, 6} and n in 0..9 tiles.  No GPU."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipdm-pytorch_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "attn_pipe_schedule.h"
using namespace ipdm::attn_pipe;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL it0 %d n %d b %d: ", it0, n, b); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main()
{
    const int starts[3] = {0, 1, 6};
    int walks = 0;
    for (int it0 : starts)
        for (int n = 0; n <= 9; ++n) {
            int b = -1;
            const int nb = barriers(n);
            // both sides run `for (b = 0; b < barriers(n); ++b)` (the consumers as first + steady + last): n + 1 barriers, none for n = 0
            CHECK(nb == (n > 0 ? n + 1 : 0), "barriers %d", nb);
            CHECK(n == 0 ? steady(n) == 0 : 1 + steady(n) + 1 == nb, "steady %d", steady(n));
            int kslot[2] = {NONE, NONE}, vslot[2] = {NONE, NONE};      // the tile each slot holds
            int kreg = NONE, vreg = NONE;                              // the tile the producers' registers hold
            int kseen = 0, vseen = 0;
            if (n > 0) kreg = k_stored(it0, n, 0);                     // (the load in front of the loop)
            int kread_prev = NONE, vread_prev = NONE;                  // what the consumers read in the interval in front of barrier b
            for (b = 0; b < nb; ++b) {
                // ---- producers, in front of barrier b: the stores fall into the consumers' interval b - 1
                const int ks = k_stored(it0, n, b), vs = v_stored(it0, n, b);
                if (ks != NONE) {
                    CHECK(ks == kreg, "K store of tile %d, registers hold %d", ks, kreg);
                    CHECK(kread_prev == NONE || slot(ks) != slot(kread_prev), "K slot %d written while tile %d is read from it", slot(ks), kread_prev);
                    kslot[slot(ks)] = ks;
                }
                if (vs != NONE) {
                    CHECK(vs == vreg, "V store of tile %d, registers hold %d", vs, vreg);
                    CHECK(vread_prev == NONE || slot(vs) != slot(vread_prev), "V slot %d written while tile %d is read from it", slot(vs), vread_prev);
                    vslot[slot(vs)] = vs;
                }
                const int kl = k_loaded(it0, n, b), vl = v_loaded(it0, n, b);
                if (kl != NONE) { CHECK(kl >= it0 && kl < it0 + n, "K load of tile %d", kl); kreg = kl; }
                if (vl != NONE) { CHECK(vl >= it0 && vl < it0 + n, "V load of tile %d", vl); vreg = vl; }
                // ---- barrier b; consumers, interval b
                const int kr = k_read(it0, n, b), vr = v_read(it0, n, b);
                CHECK(b == 0 ? (kr != NONE && vr == NONE) : b + 1 == nb ? (kr == NONE && vr != NONE) : (kr != NONE && vr != NONE), "forms: K %d V %d", kr, vr);
                if (kr != NONE) {
                    CHECK(kr == it0 + kseen, "S of tile %d out of order", kr);
                    CHECK(kslot[slot(kr)] == kr, "K slot %d holds %d, tile %d is read", slot(kr), kslot[slot(kr)], kr);
                    ++kseen;
                }
                if (vr != NONE) {
                    CHECK(vr == it0 + vseen, "P.V of tile %d out of order", vr);
                    CHECK(vr < it0 + kseen, "P.V of tile %d in front of its scores", vr);
                    CHECK(vslot[slot(vr)] == vr, "V slot %d holds %d, tile %d is read", slot(vr), vslot[slot(vr)], vr);
                    ++vseen;
                }
                kread_prev = kr;
                vread_prev = vr;
            }
            b = nb;
            CHECK(kseen == n && vseen == n, "%d scores, %d P.V of %d tiles", kseen, vseen, n);
            // nothing is touched outside the walk
            CHECK(k_stored(it0, n, nb) == NONE && v_stored(it0, n, nb + 1) == NONE && k_read(it0, n, nb) == NONE && v_read(it0, n, nb + 1) == NONE
                      && k_stored(it0, n, -1) == NONE && v_stored(it0, n, 0) == NONE && v_read(it0, n, 0) == NONE, "a tile outside the walk");
            ++walks;
        }
    std::printf("walks %d fails %d\n", walks, fails);
    return fails ? 1 : 0;
}
"""


def _host_compiler():
    for name in ("c++", "g++", "clang++"):
        p = shutil.which(name)
        if p:
            return p
    p = "/opt/rocm/lib/llvm/bin/clang++"
    return p if os.path.exists(p) else None


def test_the_ring_schedule_replayed_on_the_host(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler"
    src = tmp_path / "schedule.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "schedule"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "walks 30 fails 0" in r.stdout, r.stdout
