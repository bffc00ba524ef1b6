"""Static checks of the pair-form FFN loop with the relu inside the conversion (FD_RELU_CLAMP), on the ISA hipcc emits for gfx950.

No GPU: the benched k_mega instantiation is cross-compiled alone, as scripts/mega_isa_regions.py does, and fd_mega.hip as a whole for
the resource tuples of every instantiation.

* The relu is gone: no v_pk_max_i16 in a basic block that holds a 32x32x16 MFMA.
* Every clamped conversion is inline asm, and hipcc places no wait states for an inline-asm read of an MFMA result.  The distance has
  to hold by construction; it is counted here the way the hazard table counts it (CDNA4 ISA guide, section 4.5 "Manually Inserted
  Wait States", XDL write VGPR -> VALU read of that VGPR: number of passes + 4 on gfx950, i.e. 8 wait states behind the 4-pass
  v_mfma_f32_16x16x32_bf16 and 12 behind the 8-pass v_mfma_f32_32x32x16_bf16 -- the s_nop 7 / s_nop 11 hipcc itself pads in front of
  a compiler-generated VALU read).  One wait state per instruction in between, N + 1 for s_nop N, along EVERY backward path: the
  fall-through, every branch to a label on the way, so the loop's back-edge and its entry from the prologue both count.
* 256 VGPRs at most (two waves per SIMD), and no instantiation of k_mega spills more VGPR dwords or uses more scratch than the parent
  commit's did: profiles/mega_relu_clamp_resources.txt holds the parent's tuples beside the ones recorded for this change.  (The
  SGPR "spill" column counts SGPRs parked in VGPR lanes, not memory; it moves by single digits either way and is recorded, not
  asserted -- the convention of the earlier k_mega resource records.)

The DMA-address part of the change did not ship (hipcc does not select the saddr form of global_load_lds), so the 64-bit
address VALU in the light waves' blocks is not asserted on.
"""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")

XDL_TO_VALU_WAIT = {"v_mfma_f32_16x16x32_bf16": 8, "v_mfma_f32_32x32x16_bf16": 12}    # passes + 4 (gfx950)
MAX_WAIT = max(XDL_TO_VALU_WAIT.values())


def _tool():
    spec = importlib.util.spec_from_file_location("mega_isa_regions", os.path.join(ROOT, "scripts", "mega_isa_regions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def benched(tmp_path_factory):
    tool = _tool()
    res, asm = tool.compile_benched(tool.CSRC, str(tmp_path_factory.mktemp("isa")), "benched")
    return tool, res, tool.kernel_lines(asm)


def _regs(tok):
    """v7 -> {7}; v[2:17] -> {2..17}; anything else -> {}"""
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def _operands(ins):
    return [t.strip() for t in ins.split(None, 1)[1].split(",")] if " " in ins else []


def test_no_packed_max_beside_the_pair_mfmas(benched):
    tool, _, lines = benched
    s32 = [(n, b) for n, b in tool.blocks(lines) if any(i.startswith("v_mfma_f32_32x32x16") for i in b)]
    assert len(s32) >= 6, [n for n, _ in s32]
    for n, b in s32:
        assert not [i for i in b if i.startswith("v_pk_max_i16")], n
    clamped = [i for i in lines if i.startswith("v_cvt_pk_bf16_f32") and i.endswith("clamp")]
    # six loop instantiations (3 shapes x 2 F-halves), each with its loop body and its last steps
    assert len(clamped) >= 6 * 2 * 12, len(clamped)


def test_clamped_conversions_keep_the_xdl_write_to_valu_read_distance(benched):
    _, _, lines = benched
    label_at = {i[:-1]: k for k, i in enumerate(lines) if i.endswith(":")}
    jumps_to = {}
    for k, i in enumerate(lines):
        op = i.split()[0]
        if op.startswith("s_cbranch") or op == "s_branch":
            jumps_to.setdefault(label_at[i.split()[1]], []).append(k)

    def preds(k):
        out = list(jumps_to.get(k, [])) if lines[k].endswith(":") else []
        if k > 0 and lines[k - 1].split()[0] not in ("s_branch", "s_endpgm", "s_setpc_b64"):
            out.append(k - 1)
        return out

    checked, worst = 0, 1 << 30
    for at, ins in enumerate(lines):
        if not (ins.startswith("v_cvt_pk_bf16_f32") and ins.endswith("clamp")):
            continue
        ops = _operands(ins[:-len("clamp")].rstrip())
        src = _regs(ops[1]) | _regs(ops[2])
        assert len(src) == 2, ins
        best = {}                                   # position -> fewest wait states seen on a path from the conversion back to it
        todo = [(p, 0) for p in preds(at)]
        while todo:
            k, waited = todo.pop()
            if waited >= MAX_WAIT or best.get(k, 1 << 30) <= waited:
                continue
            best[k] = waited
            i = lines[k]
            if i.endswith(":"):
                todo += [(p, waited) for p in preds(k)]
                continue
            op = i.split()[0]
            if op.startswith("v_mfma"):
                assert op in XDL_TO_VALU_WAIT, i
                if _regs(_operands(i)[0]) & src:
                    worst = min(worst, waited - XDL_TO_VALU_WAIT[op])
                    assert waited >= XDL_TO_VALU_WAIT[op], (
                        f"{ins!r} at {at} reads the result of {i!r} at {k} after {waited} wait states, needs {XDL_TO_VALU_WAIT[op]}")
            step = int(i.split()[1]) + 1 if op == "s_nop" else 1
            todo += [(p, waited + step) for p in preds(k)]
        checked += 1
    assert checked >= 6 * 2 * 12, checked
    print(f"[isa] {checked} clamped conversions; smallest margin over the required wait states: "
          f"{'none within %d states' % MAX_WAIT if worst == 1 << 30 else worst}")


def _recorded_parent():
    """{mangled name: parent's (VGPRs, AGPRs, SGPRs, scratch, VGPR spill, SGPR spill, LDS)} from the committed record"""
    out = {}
    with open(os.path.join(ROOT, "profiles", "mega_relu_clamp_resources.txt")) as f:
        for ln in f:
            m = re.match(r"(_Z\S*k_mega\S*) \(([\d, ]+)\) -> \(([\d, ]+)\)", ln)
            if m:
                out[m.group(1)] = tuple(int(v) for v in m.group(2).split(","))
    return out


def test_registers_and_spills_not_above_the_parent(benched):
    tool, res, _ = benched
    assert res[0] <= 256, res
    parent = _recorded_parent()
    new = tool.compile_whole(tool.CSRC)
    assert parent and set(new) == set(parent), sorted(set(new) ^ set(parent))
    for name, r in sorted(new.items()):
        p = parent[name]
        assert r[0] <= 256 and r[3] <= p[3] and r[4] <= p[4], (name, p, r)
