"""The adaptive pass schedule's decision (t_start=None; Model/model.py:582-613), taken per slice: which branch every slice of a
batch takes after the ts=20 probe pass, and which slices can run the remaining passes together.  Pure Python -- no torch, no
GPU -- so that the decision is testable on its own.  The thresholds and the (t_list, eta) tables live HERE only.

The reference decides ONCE per batch: proj mode on delt.max() over the whole batch (:596-609), img mode on the single
`noise_strength` string (:582-590): diffusion.guided_reverse_process asks `schedule` for that one value.  Under its option
adaptive_per_slice every slice decides on its own value by the same thresholds and tables (`adaptive_groups`)."""
from collections import namedtuple

# branch -> (t_list, eta); proj: Model/model.py:596-609, img: :582-590
BRANCHES = {"proj": {"high": ((30, 25, 20), 0.6), "mid": ((20, 18, 15), 0.5), "low": ((15, 15, 15), 0.5)},
            "img": {"high": ((15, 15, 15), 0.6), "mid": ((15, 12, 10), 0.55), "low": ((10, 10, 10), 0.5)}}
PROJ_HIGH, PROJ_MID = 30, 4.5            # emax >= 30: high; >= 4.5: mid; else low (the reference's `>=`)

# draws of the longest branch after the probe pass (ts + 1 per pass): under adaptive_per_slice a noise source is advanced by
# this count whatever the branches were, so that what follows in a pipeline does not depend on them
MAX_DRAWS = {m: max(sum(t + 1 for t in tl) for tl, _ in b.values()) for m, b in BRANCHES.items()}

Group = namedtuple("Group", "slices t_list eta branch")


def proj_branch(emax):
    """Branch of one slice from its own maximum of the exponential map."""
    return "high" if emax >= PROJ_HIGH else ("mid" if emax >= PROJ_MID else "low")


def img_branch(noise_strength):
    """Branch of one slice from its noise_strength entry: "high", "mid", anything else ("low", None) the short schedule --
    the reference's if / elif / else."""
    return noise_strength if noise_strength in ("high", "mid") else "low"


def schedule(mode, value):
    """(t_list, eta, branch name) for ONE value: an emax in proj mode, a noise_strength entry in img mode."""
    name = proj_branch(value) if mode == "proj" else img_branch(value)
    t_list, eta = BRANCHES[mode][name]
    return list(t_list), eta, name


def adaptive_groups(mode, emax=None, noise_strength=None, batch=None):
    """The groups of a batch: slices with the same (t_list, eta), ordered by their first slice index.

    proj: `emax` is the sequence of B per-slice values.  img: `noise_strength` is one entry for all `batch` slices (a string or
    None, as the reference takes it) or a sequence of `batch` entries; a sequence of another length is refused.
    Returns a list of Group(slices, t_list, eta, branch); `slices` are batch rows in rising order."""
    if mode == "proj":
        if emax is None:
            raise ValueError("adaptive_groups('proj') needs the per-slice emax values")
        names = [proj_branch(float(v)) for v in emax]
        if batch is not None and len(names) != int(batch):
            raise ValueError("emax has %d entries for a batch of %d" % (len(names), int(batch)))
    elif mode == "img":
        if isinstance(noise_strength, (list, tuple)):
            if batch is not None and len(noise_strength) != int(batch):
                raise ValueError("noise_strength has %d entries for a batch of %d" % (len(noise_strength), int(batch)))
            names = [img_branch(v) for v in noise_strength]
        else:
            if batch is None:
                raise ValueError("adaptive_groups('img') with one noise_strength for all slices needs the batch size")
            names = [img_branch(noise_strength)] * int(batch)
    else:
        raise ValueError("mode must be 'proj' or 'img', not %r" % (mode,))
    if not names:
        raise ValueError("adaptive_groups: an empty batch")
    rows = {}
    for b, name in enumerate(names):          # dicts keep insertion order: a group's place is its first slice's
        rows.setdefault(name, []).append(b)
    table = BRANCHES[mode]
    return [Group(tuple(r), tuple(table[name][0]), table[name][1], name) for name, r in rows.items()]


def branch_names(groups):
    """The per-slice branch names of a batch, in slice order, from its groups."""
    n = sum(len(g.slices) for g in groups)
    out = [None] * n
    for g in groups:
        for b in g.slices:
            out[b] = g.branch
    return out
