"""The geometries the ART tests share (tests/test_art_geometry_host.py on the CPU, tests/test_gpu_art.py on the device), each
chosen for the code of csrc/art.hip that it reaches, with the host-side conditions that prove it does:

  S  64 x 64,  nr 128, na 120                                 the geometry the suite has always run, as control
  W  64 x 64,  nr 256, na 60                                  bins half as wide: a 16x16 tile spans 107 bins > the 64-bin LDS
                                                              window, so the three scatter loops add straight to global memory
                                                              and both back-projections take their out-of-window fallback
  R  77 x 45,  nr 160, na 72, offsets 1.3 / -0.7 cm, angle_start 12.6 deg
                                                              non-square, ragged tiles (5 x 3), every field default_geom zeroes
  G  110 x 75, nr 224, na 48                                  35 tiles: the grid barrier runs two groups, 32 + 3

Every case is built like _small() of tests/test_gpu_art.py (the reference's fan angle and detector offset kept, the bins scaled
to nr), then ny, offset_x, offset_y and angle_start are set on BOTH structs (art.ArtGeom for the library, oracle.art.Geom).

window_span() restates footprint()'s first bin `sb` (csrc/art.hip, oracle/art_oracle.c) in numpy float32; the spans and tile
counts are conditions on these inputs (tests/test_art_geometry_host.py holds them): if a geometry is edited they are checked again,
not relaxed.

The oracle results, and the oracle's own sensitivity D(g) that scales the parity bound, are computed once per process."""
import functools

import numpy as np

from ipdm_pytorch_amd import art, synth
from oracle import art as oa

NFOOT, WIN, BMAX, TILE, SYNC_GROUP = 5, 64, 8, 16, 32       # constants of csrc/art.hip (WIN and BMAX also come back from plan.info())

CASES = {
    "S": dict(nx=64, ny=64, nr=128, na=120),
    "W": dict(nx=64, ny=64, nr=256, na=60),
    "R": dict(nx=77, ny=45, nr=160, na=72, offset_x=1.3, offset_y=-0.7, angle_start=12.6),
    "G": dict(nx=110, ny=75, nr=224, na=48),
}
BASE_TOL = 5e-5     # of the maximum: the project's parity bound on S (libm-level differences in the ray tables)


def geometry(nx, ny, nr, na, offset_x=0.0, offset_y=0.0, angle_start=0.0):
    """(ArtGeom, oracle Geom, area table, view angles)."""
    kw = dict(nx=nx, nr=nr, na=na, dr=0.0010125 * 912 / nr, offset_r=-3.75 * nr / 912)
    g, go = art.default_geom(**kw), oa.geometry(**kw)
    for s in (g, go):
        s.ny, s.offset_x, s.offset_y, s.angle_start = ny, offset_x, offset_y, angle_start
    return g, go, art.area_lut(g.dx), art.view_angles(na, 360.0 / na)


@functools.lru_cache(maxsize=None)
def case(tag):
    return geometry(**CASES[tag])


def copy_geom(go, **fields):
    """A copy of a geometry struct with some fields replaced (the structs are mutable: never edit a cached one)."""
    out = type(go).from_buffer_copy(go)
    for k, v in fields.items():
        setattr(out, k, v)
    return out


def phantoms(n, nx, ny, negative=None):
    """An ellipse plus a box with a little texture, scaled to the grid; every slice differs.  `negative`: a slice whose first
    five columns are set to -0.05 (negative values take the same signed fixed-point path)."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    out = []
    for b in range(n):
        e = ((xx - nx * (0.45 + 0.015 * b)) / (nx * 0.28)) ** 2 + ((yy - ny * (0.52 - 0.01 * b)) / (ny * 0.30)) ** 2
        v = (e < 1.0).astype(np.float32) * np.float32(0.2 + 0.02 * b)
        v[ny // 3:ny // 3 + max(ny // 8, 2), nx // 2:nx // 2 + max(nx // 8, 2)] += np.float32(0.1)
        v += synth.hash_uniform((ny, nx), 700 + b) * np.float32(0.01) * (v > 0)
        out.append(v.astype(np.float32))
    out = np.stack(out)
    if negative is not None:
        out[negative, :, :5] = -0.05
    return out


def tiles(g):
    return -(-g.nx // TILE) * -(-g.ny // TILE)


def first_bins(g, betas):
    """sb of footprint() for every view and pixel, [na, ny, nx] int32 -- float32 operation by operation, as the C code."""
    f = np.float32
    beta = (np.asarray(betas, f) - f(g.angle_start)) * (f(np.pi) / f(180.0))
    cs, sn = np.cos(beta).astype(f), np.sin(beta).astype(f)
    uvt_x, uvt_y = (f(0.0) * cs - f(-1.0) * sn), (f(0.0) * sn + f(-1.0) * cs)
    uvs_x, uvs_y = (f(1.0) * cs - f(0.0) * sn), (f(1.0) * sn + f(0.0) * cs)
    xx, yy = f(g.nx) * f(g.dx) * f(0.5), f(g.ny) * f(g.dy) * f(0.5)
    # (float)((ix + 0.5) * dx - xx * 1.0f + offset): the sum is taken in double and rounded once
    x = ((np.arange(g.nx) + 0.5) * float(f(g.dx)) - float(xx) + float(f(g.offset_x))).astype(f)
    y = ((np.arange(g.ny) + 0.5) * float(f(g.dy)) - float(yy) + float(f(g.offset_y))).astype(f)
    X, Y = x[None, None, :], y[None, :, None]
    v = lambda a: a[:, None, None]
    ds = v(uvs_x) * X + v(uvs_y) * Y
    dt = v(uvt_x) * X + v(uvt_y) * Y
    gamma = np.arctan(ds / (dt + f(g.dso))).astype(f)
    assert ds.dtype == dt.dtype == gamma.dtype == f
    pos = gamma / f(g.dr) + f(0.5) * f(g.nr - 1) - f(g.offset_r)
    assert pos.dtype == f
    return np.floor(pos).astype(np.int32) - NFOOT // 2


def window_span(g, betas):
    """The largest max(sb) + NFOOT - min(sb) over all views and 16x16 tiles: the bins a tile's footprints reach from the first bin
    of its LDS window.  > WIN: the out-of-window arms run; <= WIN: they cannot."""
    sb = first_bins(g, betas)
    ty, tx = -(-g.ny // TILE), -(-g.nx // TILE)
    hi = np.full((sb.shape[0], ty * TILE, tx * TILE), np.iinfo(np.int32).min, np.int32)
    lo = np.full_like(hi, np.iinfo(np.int32).max)
    hi[:, :g.ny, :g.nx] = sb
    lo[:, :g.ny, :g.nx] = sb
    hi = hi.reshape(-1, ty, TILE, tx, TILE).max(axis=(2, 4))
    lo = lo.reshape(-1, ty, TILE, tx, TILE).min(axis=(2, 4))
    return int((hi + NFOOT - lo).max())


@functools.lru_cache(maxsize=None)
def span(tag):
    g, _, _, betas = case(tag)
    return window_span(g, betas)


def shift_case():
    """The grid of R with zero offsets and angle_start (72 views, 5 degrees apart): a volume whose content stays inside the grid
    when moved by (+3, -2) pixels, and the moved volume -- for offset == shift and angle_start == view roll."""
    g, go, lut, betas = geometry(77, 45, 160, 72)
    vol = np.zeros((2, g.ny, g.nx), np.float32)
    vol[:, 8:37, 10:64] = phantoms(2, 54, 29)
    moved = np.zeros_like(vol)
    moved[:, 6:35, 13:67] = vol[:, 8:37, 10:64]
    return g, go, lut, betas, vol, moved


# ------------------------------------------------------------------ the inputs and oracle results the GPU cases share
@functools.lru_cache(maxsize=None)
def project_inputs(tag):
    """B = 2, slice 1 with negative values."""
    g = case(tag)[0]
    v = phantoms(2, g.nx, g.ny, negative=1)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def oracle_project(tag):
    _, go, lut, betas = case(tag)
    p = oa.project(go, lut, betas, project_inputs(tag))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def recon_inputs(tag):
    """(volumes [3, ny, nx], their oracle projection [3, na, nr])."""
    g, go, lut, betas = case(tag)
    v = phantoms(3, g.nx, g.ny)
    p = oa.project(go, lut, betas, v)
    v.setflags(write=False)
    p.setflags(write=False)
    return v, p


@functools.lru_cache(maxsize=None)
def oracle_reconstruct(tag, nsart, ntv):
    _, go, lut, betas = case(tag)
    r = oa.reconstruct(go, lut, betas, recon_inputs(tag)[1], nsart, ntv, permute=False)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def sensitivity(tag):
    """D(g) = (project, reconstruct(3, 0)): the oracle's largest deviation, relative to the maximum, when every view angle moves by
    one float32 ulp, up and down -- on the inputs the parity cases use.  It measures how strongly libm-level differences in the ray
    tables (the justification of BASE_TOL) reach the result on this geometry."""
    _, go, lut, betas = case(tag)
    p0, r0 = oracle_project(tag), oracle_reconstruct(tag, 3, 0)
    dp = dr = 0.0
    for to in (np.float32(np.inf), np.float32(-np.inf)):
        b = np.nextafter(betas, to).astype(np.float32)
        dp = max(dp, float(np.abs(oa.project(go, lut, b, project_inputs(tag)) - p0).max()))
        dr = max(dr, float(np.abs(oa.reconstruct(go, lut, b, recon_inputs(tag)[1], 3, 0, permute=False) - r0).max()))
    return dp / float(np.abs(p0).max()), dr / float(np.abs(r0).max())


def bounds(tag):
    """(project, reconstruct) parity bounds of a geometry, of the maximum: BASE_TOL scaled by the oracle's own sensitivity relative
    to S and by nothing else, never below BASE_TOL."""
    d, ds = sensitivity(tag), sensitivity("S")
    return BASE_TOL * max(1.0, d[0] / ds[0]), BASE_TOL * max(1.0, d[1] / ds[1])
