"""The cache-policy bits of the shipped gfx950 code object (CPU only; the fixture of test_isa_guard.py: the code object
inside libcfk_als.so, disassembled with llvm-objdump --mcpu=gfx950).

DESIGN.md 3.5 / 10 (round 9): of the one-touch buffers of the solve launches only the REDUCE launch's partial-slot loads
measured faster with the streaming policy (`nt`); the gathers must never carry it, and the index / rating / task loads,
the factor-row and slot stores and the table preparation's source loads measured no gain or a loss and keep the default
policy. This module checks the policy bits only:
  1. in the pre-split als_solve_mfma kernels no LDS-DMA gather (global_load_lds_dwordx4) carries `nt`, and the explicit
     `s_waitcnt vmcnt(0)` still stands between every DMA and the transposed reads of its image;
  2. in every REDUCE instantiation of als_solve_mfma exactly the slot's words (4 per tile, C RHS words and the check
     word per lane) are loaded `nt`, as 4-byte loads;
  3. no other access of any als_solve_* / als_presplit_* kernel carries `nt`: an arm that comes back must come back
     with its measurement (and change this test).
"""
import re

from test_isa_guard import kernels  # noqa: F401  (the module-scoped fixture)

MFMA = re.compile(r"als_solve_mfmaILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])E")


def _nt(ops):
    return "nt" in " ".join(ops).split()


def _mfma_kernels(kernels):
    """{name: (KP, PRESPLIT, REDUCE, instructions)} of the als_solve_mfma instantiations."""
    out = {}
    for name, ins in kernels.items():
        m = MFMA.search(name)
        if m:
            out[name] = (int(m.group(1)), m.group(4) == "1", m.group(5) == "1", ins)
    assert len(out) >= 12, sorted(kernels)
    return out


def test_presplit_gathers_keep_the_default_policy_and_their_wait(kernels):
    checked = 0
    for name, (kp, presplit, reduce, ins) in _mfma_kernels(kernels).items():
        if not presplit:
            assert not any(op.startswith("global_load_lds") for op, _ in ins), name
            continue
        dma = [ops for op, ops in ins if op == "global_load_lds_dwordx4"]
        assert len(dma) >= 2 * (kp // 16) * 2, (name, len(dma))    # prologue + loop, 2 C instructions per block each
        assert not any(_nt(ops) for ops in dma), name
        pending, reads = False, 0
        for op, ops in ins:
            if op == "global_load_lds_dwordx4":
                pending = True
            elif op == "s_waitcnt" and "vmcnt(0)" in " ".join(ops).split():
                pending = False
            elif op == "ds_read_b64_tr_b16":
                reads += 1
                assert not pending, f"{name}: transposed read behind an LDS-DMA without s_waitcnt vmcnt(0)"
        assert reads >= 16, (name, reads)
        checked += 1
    assert checked >= 2, checked    # KP = 64 and KP = 128


def test_reduce_slot_loads_stream(kernels):
    checked = 0
    for name, (kp, presplit, reduce, ins) in _mfma_kernels(kernels).items():
        if not reduce:
            continue
        c = kp // 16
        slot_words = 4 * (c * (c + 1) // 2) + c + 1
        loads = [(op, ops) for op, ops in ins if re.match(r"(global|buffer|flat)_load", op)]
        nt = [op for op, ops in loads if _nt(ops)]
        assert nt == ["global_load_dword"] * slot_words, (name, len(nt), slot_words, sorted(set(nt)))
        assert not any(_nt(ops) for op, ops in ins if re.match(r"(global|buffer|flat)_(store|atomic)", op)), name
        checked += 1
    assert checked >= 3, checked    # KP = 32, 64 (two occupancies), 128


def test_nothing_else_streams(kernels):
    checked, bad = 0, []
    for name, ins in kernels.items():
        if "als_solve_" not in name and "als_presplit_" not in name:
            continue
        m = MFMA.search(name)
        if m and m.group(5) == "1":
            continue    # the REDUCE instantiations: test_reduce_slot_loads_stream
        checked += 1
        bad += [(name, op) for op, ops in ins if re.match(r"(global|buffer|flat|scratch)_", op) and _nt(ops)]
    assert checked >= 16, checked
    assert not bad, bad[:8]
