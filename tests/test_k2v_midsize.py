"""K2V's mid-size phase (csrc/align_refv.hip): introselect rounds of kOneWave < S <= kMid positions run on
an LDS copy of the segment instead of the register rows.

CPU: tests/cpp/midsize_model.cpp restates the phase (dump, rounds on relative positions, the recorded vec[nth - 1],
     hand-over to index 0, depth limit inside the phase) and compares vec[nth - 1], vec[nth], median and MAD with the
     real std::nth_element on the families below and on 2000 random short vectors.
GPU: svo_debug_robust_scale on vectors that enter the phase, through the debug kernel's round trace (every round's
     segment, pivot, Ks, #GE, #LE, cut equal to the numpy round model's, the kept segment bit-equal, a mid-size round's
     record carrying kind 2) and through the product kernel (out_len 2); median and MAD bit-equal to the oracle's
     std::nth_element.

Sizes (LayA, the layout of every vector here): the product kernel hands segments of <= 2048 positions to wave 0, the
debug kernel segments of <= 1024; both run the phase up to 7168 positions.  test_sizes_match_the_kernel_source pins
these numbers to the source.

Every case must contain a round with kOneWave < S <= kMid in the model's rounds (for the product's kOneWave, the
narrower band), or it fails instead of passing empty.  The depth-limit cases are exempt from that and instead assert
that the model runs out of depth: organ-pipe vectors do so from 7167 positions on (24 rounds leave 1665 positions; at
2049, 2050 and 4097 the numpy model, which is pinned to std::nth_element, finishes in 12-13 rounds, so there the
organ-pipe vector is an ordinary case), and the median-of-three adversary of tests/cpp/introselect_model.cpp does at
every length.
"""
import atexit
import functools
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import introselect_rounds as IR
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = np.finfo(np.float64).max
HEAD = 8
OW, OW_DBG, MID = 2048, 1024, 7168
SPECIAL = 5000  # the length whose n is chosen from the content's own cuts (nth == first / nth == last - 1)


def test_sizes_match_the_kernel_source():
    src = open(os.path.join(ROOT, "semi-direct-visual-odometry_amd", "csrc", "align_refv.hip")).read()
    assert int(re.search(r"#define SVO_ONEWAVE (\d+)", src).group(1)) == OW
    assert int(re.search(r"#define SVO_MID (\d+)", src).group(1)) == MID
    assert re.search(r"using LayADbg = Lay<RowsA, 98, 12288, true, (\d+), SVO_MID>", src).group(1) == str(OW_DBG)


def test_midsize_model_matches_std_nth_element(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "midsize"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "midsize_model.cpp")])
    r = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ok, cases, mid, heap = r.stdout.split()
    assert ok == "ok" and int(cases) > 4000 and int(mid) > 1000 and int(heap) > 0, r.stdout


# ---------------------------------------------------------------------------------------------- the cases
CONTENTS = ["normal", "integers", "equal", "ascending", "descending", "organ", "zeros", "vis1", "killer"]
LENGTHS = [("ow+1", OW + 1), ("ow+2", OW + 2), ("mid-1", MID - 1), ("mid", MID), ("mid+1", MID + 1), ("4097", 4097),
           ("nth=first", SPECIAL), ("nth=last-1", SPECIAL)]


def organ(n):
    h = (n + 1) // 2
    return np.concatenate([np.arange(h), np.arange(n - h)[::-1]]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _imodel():
    """tests/cpp/introselect_model.cpp, built once per session."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp()
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "imodel")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "introselect_model.cpp")])
    return exe


@functools.lru_cache(maxsize=None)
def killer(n):
    """The median-of-three adversary's n doubles for nth = n / 2 (tests/cpp/introselect_model.cpp), mapped into the
    residual range in order."""
    exe = _imodel()
    out = os.path.join(os.path.dirname(exe), f"k{n}.bin")
    subprocess.check_call([exe, "killer", str(n), str(n // 2), out])
    return np.fromfile(out, np.float64) / n * 500.0 - 250.0


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def make(content, n, seed):
    rng = np.random.default_rng(seed)
    if content == "normal":
        v = rng.normal(0, 8, n)
        v[np.repeat(rng.random(n // 25 + 1) < 0.2, 25)[:n]] = DBL_MAX
        if not (v < DBL_MAX).any():
            v[0] = 0.0
    elif content == "integers":
        v = np.round(rng.normal(0, 4, n))
    elif content == "equal":
        v = np.full(n, 3.0)
    elif content == "ascending":
        v = np.arange(n, dtype=np.float64)
    elif content == "descending":
        v = np.arange(n, 0, -1).astype(np.float64)
    elif content == "organ":
        v = organ(n)
    elif content == "zeros":
        v = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    elif content == "vis1":
        v = np.full(n, DBL_MAX)
        v[int(rng.integers(n))] = 1.5
    else:
        v = killer(n).copy()
    return v, int((v < DBL_MAX).sum())


def pick_n(v, want):
    """n (<= len(v)) such that some round of std::nth_element(v, n / 2) ends with nth == first (want 'first': the cut
    lands on nth and the right side is kept) or nth == last - 1 (want 'last': the cut lands on nth + 1).  Rounds
    before that one cut above len / 2 >= nth, so they keep the left side whatever nth is: follow them with
    nth = len / 2 and take the first cut that fits."""
    T = len(v) // 2
    for f0, l0, p, ks, ng, nl, cut, a in IR.rounds(v, T):
        c = cut if want == "first" else cut - 1
        if 1 <= c <= T:
            return 2 * c
        if cut <= T:
            break
    raise AssertionError("no round of this vector has a usable cut")


@functools.lru_cache(maxsize=None)
def case(content, lname):
    """(vector, n, the model's rounds of both passes, the oracle's median and MAD, depth limit reached): computed
    once, read-only."""
    n_len = dict(LENGTHS)[lname]
    v, n = make(content, n_len, seed=LENGTHS.index((lname, n_len)) * 16 + CONTENTS.index(content))
    if lname.startswith("nth=") and content not in ("vis1", "killer"):  # (those two are defined by their own n)
        n = pick_n(v, "first" if lname == "nth=first" else "last")
    nth = n // 2
    med = O.median(v, n, 0)
    x1 = np.where(v >= DBL_MAX, DBL_MAX, np.abs(v - med))
    mad = O.median(x1, n, 0)
    passes, limit = [], False
    for x in (v, x1):
        rs = []
        gen = IR.rounds(x, nth)
        try:
            while True:
                f0, l0, p, ks, ng, nl, cut, a = next(gen)
                first, last = (cut, l0) if cut <= nth else (f0, cut)
                rs.append((f0, l0, p, ks, ng, nl, cut, first, last, a[first:last].copy()))
        except StopIteration as e:
            first, last, _ = e.value
        limit = limit or last - first > 3
        passes.append(rs)
    v.setflags(write=False)
    return v, n, passes, med, mad, limit


CASES = [(c, l) for l, _ in LENGTHS for c in CONTENTS]


def in_band(rs, ow):
    return [r for r in rs if ow < r[1] - r[0] <= MID]


@pytest.mark.parametrize("content,lname", CASES, ids=[f"{c}-{l}" for c, l in CASES])
def test_cases_enter_the_phase(content, lname):
    """CPU: every case has a mid-size round in the model's rounds (product band), the depth-limit cases run out of
    depth, and the two special lengths have the round they were built for."""
    v, n, passes, med, mad, limit = case(content, lname)
    nth = n // 2
    n_len = dict(LENGTHS)[lname]
    depth_case = content == "killer" or (content == "organ" and n_len >= MID - 1)
    if depth_case:
        assert limit, "the model does not reach the depth limit"
    else:
        assert in_band(passes[0], OW), "no round with kOneWave < S <= kMid"
    if lname.startswith("nth=") and content not in ("vis1", "killer"):
        hit = [r for r in in_band(passes[0], OW) if (r[7] == nth if lname == "nth=first" else r[8] - 1 == nth)]
        assert hit, "no mid-size round ends with " + lname


def _check_trace(out, ns, v, n, passes, nrec):
    recs = out[206:].reshape(nrec, HEAD + ns)
    ri = 0
    kinds = []
    for P, rs in enumerate(passes):
        for f0, l0, p, ks, ng, nl, cut, first, last, kept in rs:
            h = recs[ri, :HEAD]
            got = (int(h[0]) % 10, int(h[1]), int(h[2]), h[3], int(h[4]), int(h[5]), int(h[6]), int(h[7]))
            print(f"round {ri}: pass {P} kind {int(h[0]) // 10} S {l0 - f0} ks {ks} cut {cut}")
            assert got == (P, f0, l0, p, ks, ng, nl, cut), f"round {ri} (pass {P}, kind {int(h[0]) // 10})"
            vec = recs[ri, HEAD:]
            bad = np.nonzero(bits(vec[first:last]) != bits(kept))[0]
            assert len(bad) == 0, f"round {ri}: kept segment differs at {(bad[:8] + first).tolist()}"
            kind = int(h[0]) // 10
            want = 0 if l0 - f0 > MID else (2 if l0 - f0 > OW_DBG else 1)
            assert kind == want, f"round {ri}: S {l0 - f0} ran as kind {kind}, expected {want}"
            kinds.append(kind)
            ri += 1
    return kinds


@pytest.mark.gpu
@pytest.mark.parametrize("content,lname", CASES, ids=[f"{c}-{l}" for c, l in CASES])
def test_k2v_midsize_rounds_match_model(content, lname):
    import svo_amd
    from svo_amd import _capi
    v, n, passes, med, mad, limit = case(content, lname)
    ns = len(v)
    nrec = 2 * (2 * int(math.log2(ns)) + 2)
    out = np.zeros(206 + nrec * (HEAD + ns))
    ctx = svo_amd.default_context()
    _capi.check(_capi.lib().svo_debug_robust_scale(ctx.handle, _capi.ptr(np.ascontiguousarray(v)), ns, n, svo_amd.SCALE_K2V,
                                                   _capi.ptr(out), len(out)))
    kinds = _check_trace(out, ns, v, n, passes, nrec)
    assert 2 in kinds, "the debug kernel ran no mid-size round"
    print("debug", out[0], out[1], "oracle", med, mad)
    assert bits([out[0], out[1]]).tolist() == bits([med, mad]).tolist()
    # the product kernel (2048-position one-wave rounds, waves 1-7 retiring after the phase)
    pm, pd = svo_amd.debug_robust_scale(np.array(v), n, impl=svo_amd.SCALE_K2V)
    print("product", pm, pd)
    assert bits([pm, pd]).tolist() == bits([med, mad]).tolist()
