"""For every guidance input of tests/test_gpu_step_fbp_accuracy.py (tests/_accuracy.py: GUIDANCE_CASES), from the CPU oracle
alone: the share of cells in each branch of the guidance curve (e <= 1.7, 1.7 < e <= 2.75, e > 2.75) and inside the exclusion
band at its jumps (|e - 1.7| <= 1e-4 * 1.7 or |e - 2.75| <= 1e-4 * 2.75), per slice, in the float64 value; whether the float32
and the float64 oracle take the same branch outside the band; and the oracle's own gate ratios.  The GPU test needs every
branch >= 1 % (where the case asks for it) and the band <= 0.1 %: run this before the device run, adjust the lesion, not the cap.

    python tools/guidance_branch_share.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _accuracy as acc      # noqa: E402


def main():
    bad = 0
    for case in acc.GUIDANCE_CASES:
        name, mode, (B, H, W), ks, amp, peak, scale, ties, want_all = case
        x, img = acc.guidance_case_inputs(case)
        for b in range(B):
            ref = acc.guidance_ref(x[b:b + 1], img[b:b + 1], mode, ks, amp)
            r, a, y32, e64, e32, _ = ref
            band = acc.band_mask(e64)
            br = acc.branch_of(e64)
            sh = [float((br == k).double().mean()) for k in range(3)] + [float(band.double().mean())]
            same = bool((acc.branch_of(e32.double())[~band] == br[~band]).all())
            ok = sh[3] <= acc.BAND_CAP and (not want_all or min(sh[:3]) >= 0.01)
            bad += not ok
            print("%-22s slice %d: branches %5.1f / %4.1f / %4.1f %%  band %.4f %%  e max %.2f  same branch outside the band: %s  "
                  "max |L32 - L64| outside %.1e  %s" % (name, b, 100 * sh[0], 100 * sh[1], 100 * sh[2], 100 * sh[3], float(e64.max()), same,
                                                       float((y32 - r)[~band].abs().max()), "ok" if ok else "NOT OK"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
