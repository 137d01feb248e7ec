"""CPU half of the ILQL loss edge suite (tests/test_gpu_ilql_edges.py):

  * the launch table restated in tests/ilql_loss_checks.py (`select`) covers, with the V list the
    GPU file runs, every instantiation of k_ilql_rows, both ends of every entry and every
    boundary of the table — so which instantiation a GPU case runs is known by reading;
  * the restated constants are the ones in csrc/ilql_rows.hip;
  * the precondition of the GPU comparisons: on every input set of the suite the fp32 oracle
    itself stays inside the bar (rtol 1e-5 / atol 1e-6) against the fp64 oracle, so a mismatch on
    the GPU cannot be blamed on the inputs."""
import os
import re

import pytest
import torch

import ilql_loss_checks as C
from ilql_loss_checks import BF16, F32

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trlx-t5_amd", "csrc",
                   "ilql_rows.hip")


def entries(dtype, split_lds):
    """entry -> [smallest V, largest V] over every V up to the first refused one."""
    out = {}
    for V in range(1, C.V_LAST[dtype] + 2):
        e = C.entry_of(C.select(dtype, V, split_lds))
        out.setdefault(e, [V, V])[1] = V
    return out


def ran(dtype, split_lds):
    """The V that run under this knob value (a split_lds = 0 case counts for split_lds = 1 where the
    knob does not change its launch)."""
    own = {V for dt, V, sl, k in C.table_cases() if dt == dtype and sl == split_lds and k == 0}
    if split_lds:
        own |= {V for V in ran(dtype, 0) if C.select(dtype, V, 0) == C.select(dtype, V, split_lds)}
    return own


def test_restated_constants_are_the_sources():
    src = open(SRC).read()
    nvs = re.search(r"kIlqlNVs\[\] = \{([^}]*)\}", src).group(1)
    assert tuple(int(x) for x in nvs.split(",")) == C.NVS
    split = {int(k) if k else 0: (int(nv), int(nl)) for k, nv, nl in
             re.findall(r"(?:case (\d)|default): hipLaunchKernelGGL\(\(k_ilql_rows<DT, (\d+), (\d+)>\)", src)}
    assert split == C.SPLITS
    assert "nvec > 512 * 16 && nvec <= 512 * (20 + 5)" in src
    assert all(nv + nl == 25 for nv, nl in C.SPLITS.values())
    assert "for (int pref : {512, kMaxThreads})" in src and "constexpr int kLineVecs = 16" in open(
        os.path.join(os.path.dirname(SRC), "common.h")).read()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_every_nv_at_512_threads(dtype):
    """(a): the V list reaches every NV of kIlqlNVs for fp32 and bf16 at <= 512 threads."""
    got = {C.select(dtype, V)[1] for V in ran(dtype, 0) if C.entry_of(C.select(dtype, V))[::3] == ("reg", 512)}
    assert got == set(C.NVS)


def test_every_1024_thread_entry_and_every_split():
    """(b): NV 10 / 12 / 13 / 16 at 1024 threads for bf16, and for fp32 with split_lds = 1 (13 and
    16 also without: the split path takes the bound 8193..12800 first), fp32 V = 50257 at
    1024 x 13, and all four split instantiations."""
    for dtype, sl, want in ((BF16, 0, {10, 12, 13, 16}), (F32, 0, {13, 16}), (F32, 1, {10, 12, 13, 16})):
        got = {C.select(dtype, V, sl)[1:] for V in ran(dtype, sl) if C.select(dtype, V, sl)[3] > 512}
        assert {nv for nv, nl, thr in got} == want and all(thr > 512 and nl == 0 for nv, nl, thr in got)
    assert C.select(F32, 50257, split_lds=1) == ("reg", 13, 0, 1024) and 50257 in ran(F32, 1)
    splits = {C.select(dt, V, sl, k)[1:3] for dt, V, sl, k in C.table_cases() if C.select(dt, V, sl, k)[0] == "split"}
    assert splits == {(20, 5), (22, 3), (21, 4), (19, 6)}
    assert C.select(F32, 50257) == ("split", 20, 5, 512)
    for k in (1, 2, 3):  # each at both ends of the split range
        assert {V for dt, V, sl, kk in C.table_cases() if kk == k} >= {32708, 51139}
    # every reachable 1024-thread entry is one of those: nothing else exists to run
    for dtype, sl in ((F32, 0), (F32, 1), (BF16, 0)):
        assert {e for e in entries(dtype, sl) if e and e[3] == 1024} == \
               {C.entry_of(C.select(dtype, V, sl)) for V in ran(dtype, sl) if C.select(dtype, V, sl)[3] > 512}


@pytest.mark.parametrize("dtype,split_lds", [(F32, 0), (F32, 1), (BF16, 0)])
def test_both_ends_of_every_entry(dtype, split_lds):
    """(c): for each entry the smallest and the largest V that map to it."""
    have = ran(dtype, split_lds)
    ent = entries(dtype, split_lds)
    assert ent.pop(None) == [C.V_LAST[dtype] + 1] * 2   # the first V past the table, and only it
    for e, (lo, hi) in ent.items():
        assert lo in have and hi in have, (e, lo, hi)
    assert len(ent) == (16 if split_lds or dtype == BF16 else 15)


def test_boundaries_and_small_rows():
    """(c): the bound on vectors 8192 | 8193 and 12800 | 12801, the last V that fits against the
    first that is refused, V in {1, 2, 3, EPV-1, EPV, EPV+1}, the oversized entries."""
    for dtype in (F32, BF16):
        epv = 16 // C.esize(dtype)
        have = ran(dtype, 0)
        assert have >= {1, 2, 3, epv - 1, epv, epv + 1}
        pairs = [(8192, 8193)] + ([(12800, 12801)] if dtype == F32 else [])
        for lo, hi in pairs:
            vlo = max(V for V in have if C.vec_bound(V, dtype) == lo)
            vhi = min(V for V in have if C.vec_bound(V, dtype) == hi)
            assert vhi == vlo + 1 and C.entry_of(C.select(dtype, vlo)) != C.entry_of(C.select(dtype, vhi))
        assert C.V_LAST[dtype] in have
        assert C.select(dtype, C.V_LAST[dtype]) == ("reg", 16, 0, 1024) and C.select(dtype, C.V_LAST[dtype] + 1) is None
        assert C.vec_bound(C.V_LAST[dtype], dtype) == 16 * 1024
    assert C.vec_bound(51139, F32) == 12800 and C.select(F32, 51139)[0] == "split"
    assert C.select(F32, 51140) == ("reg", 13, 0, 1024) and C.select(F32, 32707) == ("reg", 16, 0, 512)
    over = set()
    for dtype, sl, V in C.OVERSIZED_V:
        path, nv, nl, thr = C.select(dtype, V, sl)
        pref = 512 if thr <= 512 else 1024
        need = -(-C.vec_bound(V, dtype) // pref)
        assert need < nv and (dtype, V, sl, 0) in C.table_cases()
        over.add((dtype, pref, need, nv))
    assert over == {(dt, pref, need, nv) for dt in (F32, BF16) for pref in (512, 1024)
                    for need, nv in ((9, 10), (11, 12), (14, 16), (15, 16))}


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_locate_walks_every_element_once(dtype):
    """locate() is a bijection of the row's elements onto head / tail / (step, lane, element) for a
    misaligned row of every path; y_positions names what it says."""
    es = C.esize(dtype)
    for V, ptr in ((1031, 4096 + 16 * 15 + es), (5, 4096 + 16 - es), (C.YPOS_V[dtype][0], 8192 + C.ypos_p0(dtype))):
        sel = C.select(dtype, V)
        seen = {C.locate(ptr, V, dtype, sel, j) for j in range(V)}
        assert len(seen) == V
        _, nv, nl, thr = sel
        assert all(s[0] in ("head", "tail") or (s[1] < nv + nl and s[2] < thr) for s in seen)
    for V in C.YPOS_V[dtype]:
        sel = C.select(dtype, V, 0)
        ptr = 8192 + C.ypos_p0(dtype)
        head, nvec, tail0, tail, shift = C.row_split(ptr, V, es)
        epv = 16 // es
        assert (head, tail, shift) == (epv - 1, epv - 1, 6)
        pos = C.y_positions(ptr, V, dtype, sel)
        where = {k: C.locate(ptr, V, dtype, sel, j) for k, j in pos.items()}
        assert len(set(pos.values())) == len(pos)
        assert [where[f"head{e}"] for e in range(epv - 1)] == [("head", e) for e in range(epv - 1)]
        assert [where[f"tail{e}"] for e in range(epv - 1)] == [("tail", e) for e in range(epv - 1)]
        assert where["vec0_first"][3:] == (0, 0) and where["vec0_last"][3:] == (0, epv - 1)
        assert where["last_vec"][3] == nvec - 1 and where["step0"][:2] == ("vgpr", 0)
        _, nv, nl, thr = sel
        last = (nvec - 1 + shift) // thr
        assert where["vgpr_last_step"][:2] == ("vgpr", min(nv - 1, last)) and last >= 1
        if sel[0] == "split":
            assert where["lds_first_step"][:2] == ("lds", nv) and where["lds_last_step"][:2] == ("lds", last)
            assert last > nv
    assert C.select(F32, C.YPOS_V[F32][1])[0] == "split" and C.select(BF16, C.YPOS_V[BF16][1])[3] == 1024
    assert all(C.select(F32, V)[0] == "split" for V in C.PHASE_V[F32][1:3])


CASES = C.cpu_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_oracle_is_inside_the_bar(name):
    """The precondition: fp32 oracle against fp64 oracle at rtol 1e-5 / atol 1e-6 on the inputs of
    every case of the GPU file (bf16 cases: on the bf16-quantised inputs; the > 100k-row
    reduction case on a 16-sequence slice of the same generator)."""
    c = CASES[name]()
    w32 = c.want(torch.float32)
    C.check64(w32, c.want(torch.float64), dtype=F32)
    assert all(bool(torch.isfinite(w32[1][k])) for k in C.KEYS)
