"""CPU-only checks of the ILQL heads module: the reference's state_dict loads into ILQLHeads
with strict=True (names and shapes from tests/golden/ilql_heads_keys.npz, written by
tests/golden/make_golden_ilql_heads.py from the reference's ILQLHeads), CPU tensors are
refused, polyak_update validates its arguments, and the header declares the new exports with
the struct layout the ctypes mirror assumes."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import trlx_t5_amd as P
from trlx_t5_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trlx_t5_amd.h")


def reference_entries(z, two_qs):
    k = f"two_qs{int(two_qs)}"
    names = [str(n) for n in z[f"{k}/names"]]
    shapes = [tuple(int(d) for d in s[:n]) for s, n in zip(z[f"{k}/shapes"], z[f"{k}/ndim"])]
    return names, shapes


@pytest.mark.parametrize("two_qs", [False, True])
def test_reference_state_dict_loads_strict(golden, two_qs):
    z = golden("ilql_heads_keys")
    H, V = int(z["hidden_size"]), int(z["vocab_size"])
    names, shapes = reference_entries(z, two_qs)
    assert len(names) == (4 + 4 + 4) * (2 if two_qs else 1) - (4 if two_qs else 0)
    g = torch.Generator().manual_seed(1)
    sd = {n: torch.randn(s, generator=g) for n, s in zip(names, shapes)}
    heads = P.ILQLHeads(P.ILQLConfig(two_qs=two_qs), H, V)
    assert list(heads.state_dict()) == names  # the reference's names, in its order
    res = heads.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for n, t in heads.state_dict().items():
        assert torch.equal(t, sd[n])
    # the reference's freezing: target heads carry no gradient, the others do
    for n, p in heads.named_parameters():
        assert p.requires_grad == (not n.startswith("target_q_heads")), n
    # ILQLConfig.heads is the reference's factory (ilql_models.py:49-50)
    assert list(P.ILQLConfig(two_qs=two_qs).heads(H, V).state_dict()) == names


def test_target_heads_start_as_copies_of_the_q_heads():
    heads = P.ILQLHeads(P.ILQLConfig(), 8, 11)
    for q, t in zip(heads.q_heads.parameters(), heads.target_q_heads.parameters()):
        assert torch.equal(q, t) and q.data_ptr() != t.data_ptr()


def test_heads_refuse_cpu_tensors():
    B, L, H, V = 2, 5, 8, 11
    heads = P.ILQLHeads(P.ILQLConfig(), H, V)
    hs = torch.randn(B, L, H)
    ids = torch.zeros(B, L, dtype=torch.long)
    six, aix = torch.arange(L).repeat(B, 1), torch.arange(L - 1).repeat(B, 1)
    with pytest.raises(ValueError, match="ROCm"):
        heads.forward_for_loss(hs, ids, six, aix)
    with pytest.raises(ValueError, match="ROCm"):
        heads.sync_target_q_heads()
    with pytest.raises(ValueError, match="ROCm"):
        P.ilql_target_q_at_actions([torch.randn(B, L - 1, 4)], [torch.randn(V, 4)], None, ids, aix)
    with pytest.raises(ValueError, match="ROCm"):
        P.polyak_update([torch.zeros(3)], [torch.ones(3)], 0.5)
    # the plain forward is torch: it runs anywhere and returns the reference's shapes
    qs, tqs, vs = heads(hs, six, aix)
    assert len(qs) == len(tqs) == 2 and tuple(qs[0].shape) == tuple(tqs[1].shape) == (B, L - 1, V)
    assert tuple(vs.shape) == (B, L, 1)


def test_polyak_update_argument_validation():
    t, s = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(ValueError, match="targets but"):
        P.polyak_update([t, t], [s], 0.5)
    with pytest.raises(ValueError, match="source is"):
        P.polyak_update([t], [s.bfloat16()], 0.5)
    with pytest.raises(ValueError, match="shape"):
        P.polyak_update([t], [torch.ones(3, 4)], 0.5)
    with pytest.raises(ValueError, match="unsupported dtype"):
        P.polyak_update([t.double()], [s.double()], 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        P.polyak_update([t.t()], [s.t()], 0.5)
    assert torch.equal(t, torch.zeros(4, 3))


def test_target_q_argument_validation():
    ids, aix = torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long)
    z, w = torch.randn(2, 3, 4), torch.randn(7, 4)
    with pytest.raises(ValueError, match="one or two"):
        P.ilql_target_q_at_actions([z, z, z], [w, w, w], None, ids, aix)
    with pytest.raises(ValueError, match="one or two"):
        P.ilql_target_q_at_actions([z, z], [w], None, ids, aix)


def test_loss_refuses_mixed_target_forms_before_touching_the_device():
    """The form check of ILQLConfig.loss / ILQLHotPath.step is host logic."""
    from trlx_t5_amd.ilql import _tq_gathered
    B, A, V = 2, 3, 5
    full, at = torch.zeros(B, A, V), torch.zeros(B, A)
    assert _tq_gathered([full, full], B, A, V) is False
    assert _tq_gathered([at, at[..., None]], B, A, V) is True
    with pytest.raises(ValueError, match="mixes"):
        _tq_gathered([full, at], B, A, V)
    with pytest.raises(ValueError, match="shape"):
        _tq_gathered([torch.zeros(B, A + 1)], B, A, V)
    assert _tq_gathered([torch.zeros(B, A, 1)], B, A, 1) is False  # V == 1: a full row


def test_header_declares_the_new_exports():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("trlx_ilql_tq_at_actions", "trlx_polyak_update"):
        assert re.search(rf"^int {name}\(", txt, flags=re.M), name
        assert name in _lib.SIGNATURES
    assert re.search(r"\bint tq_gathered;\s*\} trlx_ilql_args;", txt)
    assert _lib.IlqlArgs._fields_[-1][0] == "tq_gathered"
    m = re.search(r"#define TRLX_POLYAK_MAX_TENSORS (\d+)", txt)
    assert m and int(m.group(1)) == _lib.POLYAK_MAX_TENSORS
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
        assert {"trlx_ilql_tq_at_actions", "trlx_polyak_update"} <= set(re.findall(r"\bT (trlx_\w+)", out))


def test_tq_args_layout_matches_header(tmp_path):
    """The ctypes mirror of trlx_ilql_tq_args has the C compiler's field offsets."""
    fields = [f[0] for f in _lib.IlqlTqArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trlx_t5_amd.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(trlx_ilql_tq_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(trlx_ilql_tq_args));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [getattr(_lib.IlqlTqArgs, f).offset for f in fields] + [ctypes.sizeof(_lib.IlqlTqArgs)]
