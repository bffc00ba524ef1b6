#!/usr/bin/env python
"""Static ISA report of the persistent kernel (k_mega, fd_mega_kernel.h), cross-compiled for gfx950 -- no GPU needed.

Two compiles per source tree, with the Makefile's flags:
  * fd_mega.hip as a whole (-Rpass-analysis=kernel-resource-usage): the resource tuple of every k_mega instantiation,
  * a one-file translation unit that takes the address of the benched instantiation alone (--cuda-device-only -S): its ISA,
    cut into the regions between s_barrier instructions (text order) and into basic blocks.
Given --parent DIR (a csrc/ directory of the parent commit, e.g. from `git archive`), both are compared and the
requirements of a change that only removes control flow are checked (printed as OK / FAIL lines at the end).

usage: python scripts/mega_isa_regions.py [--parent DIR] [--skip-whole] [-o profiles/NAME.txt]"""
import argparse, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fourierdiffusion_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-fno-honor-nans", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function"]
BENCHED = "k_mega<3, 5, 3, 4, ShapeStatic<100, 72, 12, 12, 2, 3, 2, 10, 2048, 1>, 8, false>"
ONE_TU = '#include "fd_mega.h"\n#include "fd_mega_kernel.h"\nvoid* fd_benched_kernel() { return (void*)%s; }\n' % BENCHED


def resources(stderr):
    """{mangled name: (VGPRs, AGPRs, SGPRs, scratch B/lane, VGPR spill, SGPR spill, LDS)} from the resource-usage remarks"""
    out, name, cur = {}, None, {}
    keys = [("VGPRs", r" VGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("SGPRs", r"TotalSGPRs: (\d+)"),
            ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"),
            ("lds", r"LDS Size \[bytes/block\]: (\d+)")]
    for ln in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name, cur = m.group(1), {}
        for k, pat in keys:
            m = re.search(pat, ln)
            if m and name:
                cur[k] = int(m.group(1))
        if name and len(cur) == len(keys):
            out[name] = tuple(cur[k] for k, _ in keys)
            name = None
    return out


def compile_whole(csrc):
    r = subprocess.run([HIPCC, *FLAGS, "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(csrc, "fd_mega.hip"), "-o", "/dev/null"], capture_output=True, text=True, cwd=csrc)
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    return {k: v for k, v in resources(r.stderr).items() if "k_mega" in k}


def compile_benched(csrc, tmp, tag):
    src, asm = os.path.join(tmp, tag + ".hip"), os.path.join(tmp, tag + ".s")
    with open(src, "w") as f:
        f.write(ONE_TU)
    r = subprocess.run([HIPCC, *FLAGS, "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", src, "-o", asm], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    res = [v for k, v in resources(r.stderr).items() if "k_mega" in k]
    return res[0], open(asm).read()


def kernel_lines(asm):
    """instructions and labels of the k_mega function, comments stripped"""
    out, on = [], False
    for ln in asm.splitlines():
        if re.match(r"_Z\w*6k_mega\w*:", ln):
            on = True
            continue
        if on and ln.startswith(".Lfunc_end"):
            break
        if not on:
            continue
        ln = ln.split(";")[0].rstrip()
        if not ln.strip():
            continue
        if re.match(r"\.LBB\d+_\d+:", ln):
            out.append(ln.strip())
        elif ln[0] in " \t" and not ln.strip().startswith("."):
            out.append(ln.strip())
    return out


def count(ins):
    c = dict(n=0, valu=0, mfma=0, mfma32=0, exp=0, br=0, execr=0, scr=0, ds=0, glb=0)
    for i in ins:
        if i.endswith(":"):
            continue
        op = i.split()[0]
        c["n"] += 1
        if op.startswith("v_mfma"):
            c["mfma"] += 1
            c["mfma32"] += "32x32" in op
        elif op.startswith("v_"):
            c["valu"] += 1
            c["exp"] += op.startswith("v_exp_f32")
        elif op.startswith("s_cbranch") or op == "s_branch":
            c["br"] += 1
        elif re.match(r"s_\w+_saveexec", op):
            c["execr"] += 1
        elif op.startswith("scratch_"):
            c["scr"] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith("global_") or op.startswith("buffer_"):
            c["glb"] += 1
    return c


def regions(lines):
    out, cur = [], []
    for i in lines:
        cur.append(i)
        if i.startswith("s_barrier"):
            out.append(cur)
            cur = []
    out.append(cur)
    return out


def blocks(lines):
    out, cur, name = [], [], "entry"
    for i in lines:
        if i.endswith(":"):
            out.append((name, cur))
            name, cur = i[:-1], []
        else:
            cur.append(i)
    out.append((name, cur))
    return out


def fmt(c):
    return ("n %4d valu %4d mfma %3d (32x32 %3d) exp %3d branch %3d exec %3d scratch %2d ds %3d glb %3d" %
            (c["n"], c["valu"], c["mfma"], c["mfma32"], c["exp"], c["br"], c["execr"], c["scr"], c["ds"], c["glb"]))


def report(tag, res, asm, P):
    lines = kernel_lines(asm)
    P("## %s: benched instantiation %s" % (tag, res))
    tot = count(lines)
    P("whole kernel: " + fmt(tot) + "  basic blocks %d" % sum(1 for i in lines if i.endswith(":")))
    P("# regions between barriers, text order")
    for k, r in enumerate(regions(lines)):
        P("region %2d: %s" % (k, fmt(count(r))))
    # item-2 sub-regions: out-proj + LN1 = the tail of the units' region behind its last weight DMA issue (issue_ffn sits right in
    # front of the W_o loads); combine + LN2 = the MFMA-free regions with the exchange reads (one per F-half instantiation)
    owner = []
    for k, r in enumerate(regions(lines)):
        c = count(r)
        if c["exp"] > 0:
            last = max(j for j, i in enumerate(r) if i.startswith("global_load_lds"))
            owner.append(("out-proj + LN1 (region %d behind its last DMA issue)" % k, r[last + 1:]))
        elif c["mfma"] == 0 and c["ds"] >= 30 and c["valu"] >= 250:
            owner.append(("combine + LN2 (region %d)" % k, r))
    P("# owner-phase sub-regions (item 2: no exec-mask region; reads = ds_read in front of the first lgkmcnt wait)")
    for name, r in owner:
        first_wait = next((j for j, i in enumerate(r) if "lgkmcnt" in i), len(r))
        P("%-52s %s reads ahead %2d" % (name, fmt(count(r)), sum(1 for i in r[:first_wait] if i.startswith("ds_read"))))
    hot = [(n, b) for n, b in blocks(lines) if count(b)["exp"] >= 8]
    P("# unit hot blocks (>= 8 v_exp_f32)")
    for n, b in hot:
        P("%-10s %s" % (n, fmt(count(b))))
    s32 = [(n, b) for n, b in blocks(lines) if count(b)["mfma32"] > 0]
    P("# FFN-loop blocks (hold a 32x32x16 MFMA)")
    for n, b in s32:
        P("%-10s %s" % (n, fmt(count(b))))
    return hot, s32, owner


def norm_text(b):
    """instruction text with branch targets blanked (labels are renumbered by any change elsewhere)"""
    return [re.sub(r"\.LBB\d+_\d+", ".L", i) for i in b]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="csrc/ directory of the parent commit")
    ap.add_argument("--skip-whole", action="store_true", help="benched instantiation only (5 s instead of minutes)")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    buf = []

    def P(s=""):
        print(s)
        buf.append(s)
    P("# " + HIPCC.split("/")[-1] + " " + " ".join(FLAGS) + "; benched instantiation alone with --cuda-device-only -S")
    P("# tuple: (VGPRs, AGPRs, TotalSGPRs, scratch bytes/lane, VGPR spill, SGPR spill, LDS bytes/block)")
    ok = True

    def check(name, cond, detail=""):
        nonlocal ok
        ok = ok and cond
        P("%s  %s %s" % ("OK  " if cond else "FAIL", name, detail))
    with tempfile.TemporaryDirectory() as tmp:
        trees = ([("parent", a.parent)] if a.parent else []) + [("new", CSRC)]
        rep = {}
        for tag, csrc in trees:
            res, asm = compile_benched(csrc, tmp, tag)
            rep[tag] = (res,) + report(tag, res, asm, P)
            P()
        whole = {}
        if not a.skip_whole:
            for tag, csrc in trees:
                whole[tag] = compile_whole(csrc)
            P("## every k_mega instantiation of fd_mega.hip" + (" (parent -> new)" if a.parent else ""))
            for k in sorted(whole["new"]):
                if a.parent:
                    P("%s %s -> %s" % (k, whole["parent"].get(k), whole["new"][k]))
                else:
                    P("%s %s" % (k, whole["new"][k]))
            P()
    P("## requirements")
    res, hot, s32, owner = rep["new"]
    check("benched kernel at 256 VGPRs", res[0] == 256, str(res))
    check("spill <= 43 dwords, scratch <= 96 B/lane", res[4] <= 43 and res[3] <= 96)
    check("no scratch instruction in the unit hot blocks or the FFN-loop blocks", all(count(b)["scr"] == 0 for _, b in hot + s32))
    check("out-proj + LN1 and both combine + LN2 regions hold no exec-mask region", len(owner) == 3 and all(count(r)["execr"] == 0 for _, r in owner),
          str([count(r)["execr"] for _, r in owner]))
    comb = [r for n, r in owner if n.startswith("combine")]
    ahead = [sum(1 for i in r[:next((j for j, i in enumerate(r) if "lgkmcnt" in i), len(r))] if i.startswith("ds_read")) for r in comb]
    check("combine: at least 8 LDS reads issued in front of the first wait", bool(ahead) and min(ahead) >= 8, str(ahead))
    if a.parent:
        _, phot, ps32, _ = rep["parent"]
        check("unit hot blocks: non-MFMA VALU not above the parent's", len(hot) == len(phot) and
              all(count(b)["valu"] <= count(pb)["valu"] for (_, b), (_, pb) in zip(hot, phot)),
              str([(count(pb)["valu"], count(b)["valu"]) for (_, b), (_, pb) in zip(hot, phot)]))
        same = len(s32) == len(ps32) and all(norm_text(b) == norm_text(pb) for (_, b), (_, pb) in zip(s32, ps32))
        check("FFN-loop blocks: instruction text unchanged", same,
              "" if same else str([(len(pb), len(b), sum(x != y for x, y in zip(norm_text(b), norm_text(pb))))
                                   for (_, b), (_, pb) in zip(s32, ps32)]) + " (parent n, new n, differing lines)")
        ops = lambda b: sorted(i.split()[0] for i in b)
        same_ops = [ops(b) == ops(pb) for (_, b), (_, pb) in zip(s32, ps32)]
        P("info  FFN-loop blocks with the same multiset of opcodes as the parent's (register names and order aside): %d of %d  %s" %
          (sum(same_ops), len(same_ops), "".join("=" if x else "x" for x in same_ops)))
        if whole:
            worse = [k for k in whole["new"] if k in whole["parent"] and
                     (whole["new"][k][3] > whole["parent"][k][3] or whole["new"][k][4] > whole["parent"][k][4])]
            check("no instantiation with more VGPR spill or scratch than the parent", not worse, " ".join(worse))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(buf) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
