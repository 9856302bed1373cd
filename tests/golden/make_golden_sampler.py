"""Generates tests/golden/random_sampler.json by IMPORTING THE REFERENCE's Utils/sampler.py (read-only, from
oracle.ref_shim.REFERENCE_ROOT) and listing its RandomSampler's index sequences on the CPU.

Run in the build container only:   python tests/golden/make_golden_sampler.py
The fixture is data: the constructor arguments of each case and the indices the reference's sampler yields.  Nothing here
copies reference source.
"""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "random_sampler.json")
# (len(dataset), batch_size, num_iter, restore_iter, seed)
CASES = [(10, 4, 7, 0, 0), (10, 4, 7, 3, 0), (12, 4, 6, 0, 0), (12, 4, 6, 2, 0), (7, 2, 10, 0, 0), (7, 2, 10, 4, 5), (6, 2, 6, 0, 0),
         (6, 2, 6, 3, 0), (5, 1, 12, 7, 0)]


def main():
    # the reference hands its dataset to Sampler.__init__, which current torch no longer takes: let the base class accept it,
    # so that the reference's own __init__ and __iter__ run unchanged
    import torch.utils.data.sampler as tsampler
    tsampler.Sampler.__init__ = lambda self, *args, **kwargs: None
    spec =importlib.util.spec_from_file_location("ref_sampler", os.path.join(ref_shim.REFERENCE_ROOT, "Utils", "sampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = []
    for n, bs, num_iter, restore, seed in CASES:
        s = mod.RandomSampler(list(range(n)), batch_size=bs, num_iter=num_iter, restore_iter=restore, seed=seed)
        idx = [int(i) for i in s]
        assert len(idx) == len(s)
        out.append(dict(n=n, batch_size=bs, num_iter=num_iter, restore_iter=restore, seed=seed, indices=idx))
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote %s (%d cases)" % (OUT, len(out)))


if __name__ == "__main__":
    main()
