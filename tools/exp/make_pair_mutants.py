"""Mutants of the five bf16 x 6 kernels (results wrong on purpose): does the suite notice a lost piece pair or a wrong device split?
    python tools/exp/make_pair_mutants.py [name ...]     ->  tools/abl/pairs/<name>.so  (sources: tools/exp/abl_pairs/<name>/)
    python tools/exp/run_pair_mutants.py                 ->  profiles/r07_bf16x6_pair_mutants.txt
Per kernel (gemm = gemm_bf.hip, narrow = narrow_bf.hip, w43 = conv_wino.hip's BF path, w54 = conv_wino54_kernel.h <BF>):
  <kernel>_pair_<ab>   the MFMA of pair (activation piece a, weight piece b) gets a zero activation operand (hh hm mh hl lh mm)
  <kernel>_split_l0    the device split writes l = 0
  <kernel>_split_trunc the device split truncates to bf16 instead of rounding to nearest even
The attention kernel (attention_bf_kernel.h, the full entries of attention_bf.hip) has two products, twelve pair MFMAs: attn_qk_pair_<ab> ((K piece, Q piece), the K operand
zeroed), attn_pv_pair_<ab> ((V piece, P piece), the P operand zeroed, both output halves), and one split for all four operands:
attn_qk_split_l0 / attn_qk_split_trunc.
The split mutants edit a copy of the shared bf16x6.h next to the kernel's source: only that kernel is built against it.
An operand is zeroed, no instruction deleted: addressing and register allocation stay the product's.  Built with build.py's flags
for the file (-fno-slp-vectorize where the product has it) against the product's other objects (flowhigh_amd/build/, run
`python -m flowhigh_amd.build` first); a mutant whose kernels need scratch beyond build.MAX_SCRATCH_BYTES is rejected, as the
product build rejects such a kernel."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import build as B         # noqa: E402

CSRC = ROOT / "flowhigh_amd" / "csrc"
SRC_DIR = ROOT / "tools" / "exp" / "abl_pairs"
LIB_DIR = ROOT / "tools" / "abl" / "pairs"
PAIRS = ["hh", "hm", "mh", "hl", "lh", "mm"]        # (activation piece, weight piece)
TRUNC = "  return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u);\n"


def one(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


def split(arg, l_zero="0u"):
    """bf16x6.h with its split mutated: l = l_zero, or a truncating pack"""
    t = (CSRC / "bf16x6.h").read_text()
    if arg == "l0":
        return {"bf16x6.h": one(t, "lp[i] = bf16_pack(ra - bf16_lo(mp[i]), rb - bf16_hi(mp[i]));", f"lp[i] = {l_zero};")}
    return {"bf16x6.h": one(t, "  const bf16x2 v = {(__bf16)a, (__bf16)b};\n  return __builtin_bit_cast(unsigned, v);\n", TRUNC)}


ZERO = "__builtin_bit_cast(bf16x8, (u32x4){0u, 0u, 0u, 0u})"


def gemm(kind, arg):
    t = (CSRC / "gemm_bf.hip").read_text()
    if kind == "split":
        return {"gemm_bf.hip": t, **split(arg)}
    # schedule kBf16x6SmallFirst: (l h) (h l) (m m) (m h) (h m) (h h) as (A piece, W piece)
    pp = ["lh", "hl", "mm", "mh", "hm", "hh"].index(arg)
    return {"gemm_bf.hip": one(t, "__builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt][s.a], b[nt][s.b]",
                               f"__builtin_amdgcn_mfma_f32_32x32x16_bf16(pp == {pp} ? {ZERO} : a[mt][s.a], b[nt][s.b]")}


def narrow(kind, arg):
    t = (CSRC / "narrow_bf.hip").read_text()
    if kind == "split":
        return {"narrow_bf.hip": t, **split(arg)}
    pp = ["lh", "hl", "mm", "mh", "hm", "hh"].index(arg)          # as gemm_bf.hip, (sample piece, weight piece)
    return {"narrow_bf.hip": one(t, "__builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][s.a],",
                                 f"__builtin_amdgcn_mfma_f32_16x16x32_bf16(pp == {pp} ? {ZERO} : a[i][s.a],")}


def w43(kind, arg):
    t = (CSRC / "conv_wino.hip").read_text()
    if kind == "split":                  # (l = 0 * x: not folded, the register use stays the product's)
        return {"conv_wino.hip": t, **split(arg, "bf16_pack(0.f * (ra - bf16_lo(mp[i])), 0.f * (rb - bf16_hi(mp[i])))")}
    # schedule kBf16x6SmallFirst as (weight piece, activation piece)
    pp = ["lh", "hl", "mm", "mh", "hm", "hh"].index(arg[1] + arg[0])
    # (a zero the compiler cannot see, made in a vector register by an empty asm: with a constant zero it re-schedules this
    # loop and the 64 x 512 and 128 x 256 tiles spill)
    old = "t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a3[mt][s.a]), __builtin_bit_cast(bf16x8, bp[s.b]),"
    new = (f"unsigned z = 0u;\n                if (pp == {pp}) asm volatile(\"\" : \"+v\"(z));\n"
           "                t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a3[mt][s.a]), "
           f"pp == {pp} ? __builtin_bit_cast(bf16x8, (u32x4){{z, z, z, z}}) : __builtin_bit_cast(bf16x8, bp[s.b]),")
    return {"conv_wino.hip": one(t, old, new)}


def w54(kind, arg):
    t = (CSRC / "conv_wino54_kernel.h").read_text()
    files = {"conv_wino54_bf.hip": (CSRC / "conv_wino54_bf.hip").read_text()}
    if kind == "split":                  # (the kernel header next to the mutated bf16x6.h: its quoted include finds that one)
        return {**files, "conv_wino54_kernel.h": t, **split(arg)}
    # schedule kBf16x6AMajor (W piece, activation piece): (h h) (h m) (h l) (m h) (m m) (l h)
    pp = ["hh", "mh", "lh", "hm", "mm", "hl"].index(arg)
    t = one(t, "__builtin_bit_cast(bf16x8, bp[s.b]), acc[mt][nt], 0, 0, 0);",
            f"pp == {pp} ? {ZERO} : __builtin_bit_cast(bf16x8, bp[s.b]), acc[mt][nt], 0, 0, 0);")
    return {**files, "conv_wino54_kernel.h": t}


def attn_qk(kind, arg):
    t = (CSRC / "attention_bf_kernel.h").read_text()          # (the kernel is in the header, as w54's: the full entries are built against it)
    files = {"attention_bf.hip": (CSRC / "attention_bf.hip").read_text()}
    if kind == "split":
        return {**files, "attention_bf_kernel.h": t, **split(arg)}
    pp = ["lh", "hl", "mm", "mh", "hm", "hh"].index(arg)          # kBf16x6SmallFirst as (K piece, Q piece)
    # (a zero the compiler cannot see, as in w43: with a constant zero the SPLIT = 1 kernel of some pairs spills 5 registers)
    return {**files, "attention_bf_kernel.h": one(t, "        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[c.a],",
                                    f"        unsigned z = 0u;\n        if (pp == {pp}) asm volatile(\"\" : \"+v\"(z));\n"
                                    f"        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pp == {pp} ? as_bf((u32x4){{z, z, z, z}}) : kf[c.a],")}


def attn_pv(kind, arg):
    t = (CSRC / "attention_bf_kernel.h").read_text()
    pp = ["lh", "hl", "mm", "mh", "hm", "hh"].index(arg)          # kBf16x6SmallFirst as (V piece, P piece)
    t = one(t, "        S.o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0[c.a],",
            f"        unsigned z = 0u;\n        if (pp == {pp}) asm volatile(\"\" : \"+v\"(z));\n"
            "        S.o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0[c.a],")
    for v in ("v0", "v1"):
        t = one(t, f"__builtin_amdgcn_mfma_f32_32x32x16_bf16({v}[c.a], as_bf(pq[c.b]),",
                f"__builtin_amdgcn_mfma_f32_32x32x16_bf16({v}[c.a], pp == {pp} ? as_bf((u32x4){{z, z, z, z}}) : as_bf(pq[c.b]),")
    return {"attention_bf.hip": (CSRC / "attention_bf.hip").read_text(), "attention_bf_kernel.h": t}


KERNELS = {"gemm": (gemm, "gemm_bf.hip"), "narrow": (narrow, "narrow_bf.hip"), "w43": (w43, "conv_wino.hip"),
           "w54": (w54, "conv_wino54_bf.hip"), "attn_qk": (attn_qk, "attention_bf.hip"), "attn_pv": (attn_pv, "attention_bf.hip")}
MUTANTS = [(f"{k}_pair_{p}", k, "pair", p) for k in KERNELS for p in PAIRS] + \
          [(f"{k}_split_{s}", k, "split", s) for k in KERNELS if k != "attn_pv" for s in ("l0", "trunc")]


def build(name, kernel, kind, arg):
    make, src = KERNELS[kernel]
    files = make(kind, arg)
    d = SRC_DIR / name
    d.mkdir(parents=True, exist_ok=True)
    for f, text in files.items():
        (d / f).write_text(text)
    obj = d / (src + ".o")
    cmd = [B.os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *B.FLAGS, *B.EXTRA_FLAGS.get(src, []), *B.RESOURCE_FLAGS,
           f"-I{CSRC}", "-c", str(d / src), "-o", str(obj)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        raise RuntimeError(f"{name}: hipcc failed\n{p.stderr[-3000:]}")
    spills = {k: r["ScratchSize"] for k, r in B.parse_resource_remarks(p.stderr).items() if r.get("ScratchSize", 0) > B.MAX_SCRATCH_BYTES}
    if spills:
        raise RuntimeError(f"{name}: rejected, kernels spill: {spills}")
    others = [str(ROOT / "flowhigh_amd" / "build" / (s + ".o")) for s in B.SOURCES if s != src]
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    subprocess.check_call([cmd[0], "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(LIB_DIR / f"{name}.so"), *others, str(obj)])
    obj.unlink()
    return LIB_DIR / f"{name}.so"


if __name__ == "__main__":
    from concurrent.futures import ThreadPoolExecutor
    want = [m for m in MUTANTS if not sys.argv[1:] or m[0] in sys.argv[1:]]
    with ThreadPoolExecutor(8) as ex:
        for m, f in zip(want, [ex.submit(build, *m) for m in want]):
            print(f.result().relative_to(ROOT), flush=True)
