"""Canonical text and sha256 of the vocoder's launch plans, built on the CPU (no GPU): every argument a launch receives, every
descriptor struct field by field, the ragged plans' descriptor blob decoded at its offsets (structs, run maps, tile lists),
the plan totals bench.py reads and the byte size the plan caches recorded.  Every address (tensor data_ptr, c_void_p field,
split-K slice address) is printed as b<buffer number in order of first appearance>+<byte offset>; one that lies in no tensor
reachable from the model or the plan is printed as UNKNOWN and counted.  Two commits whose dumps are equal enqueue the same
launches.  Steps are read by position and type only, so the file runs unchanged on commits with other step classes.
    python tools/plan_dump.py [--out plans.txt]      (prints the digest and the UNKNOWN count)"""
import argparse
import bisect
import ctypes as C
import hashlib
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowhigh_amd import hip, synth               # noqa: E402
from flowhigh_amd.vocoder import Vocoder          # noqa: E402

CONFIGS = ("SYNTH_CFG", "ALT_CFG", "ALT2_CFG", "ALT3_CFG", "ODD_CFG", "NK4_CFG", "NK5_AMP2_CFG", "PAD_CFG")
FORMS = ("bf16x6", "winograd", "direct")
SHAPES = ((1, 7), (1, 50), (1, 333), (2, 40), (1, 1000))
RAGGED = ([50, 333, 50, 120], [200, 200])
# merged step kind -> (descriptor struct, (offset, count, element type) of a second array in the blob, by step position)
RAGGED_DESC = {"rwino": (hip.WinoGroup, (8, 9, C.c_int32)), "rconv": (hip.ConvGroup, None), "rconvt": (hip.ConvGroup, None),
               "ramp": (hip.AmpGroup, (3, 4, C.c_int32 * 4)), "ract": (hip.ActGroup, None), "rsum": (hip.SumJob, None)}


def _storages(obj, seen, out):
    """(address, bytes) of every tensor storage reachable from obj (the walk of hip._tensor_bytes)."""
    if isinstance(obj, torch.Tensor):
        st = obj.untyped_storage()
        if st.data_ptr() not in seen and st.nbytes():
            seen.add(st.data_ptr())
            out.append((st.data_ptr(), st.nbytes()))
    elif isinstance(obj, (str, bytes, int, float, bool, type(None), type)) or ("id", id(obj)) in seen:
        return
    else:
        seen.add(("id", id(obj)))
        if isinstance(obj, (dict, list, tuple, set)) or hasattr(obj, "__dict__"):
            for v in (obj.values() if isinstance(obj, dict) else obj if isinstance(obj, (list, tuple, set)) else vars(obj).values()):
                _storages(v, seen, out)


class Addresses:
    """address -> 'b<n>+<offset>', buffers numbered in order of first appearance."""

    def __init__(self, *roots):
        found = []
        _storages(roots, set(), found)
        self.bufs = sorted(found)
        self.starts = [a for a, _ in self.bufs]
        self.number, self.unknown = {}, 0

    def __call__(self, addr):
        if not addr:
            return "null"
        i = bisect.bisect_right(self.starts, addr) - 1
        if i < 0 or addr >= self.bufs[i][0] + self.bufs[i][1]:
            self.unknown += 1
            return "UNKNOWN"
        return f"b{self.number.setdefault(i, len(self.number))}+{addr - self.bufs[i][0]}"


def struct_text(s, addr):
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.c_void_p:
            v = addr(v)
        elif isinstance(v, C.Structure):
            v = struct_text(v, addr)
        elif isinstance(v, C.Array):
            v = [struct_text(e, addr) if isinstance(e, C.Structure) else addr(e) if typ._type_ is C.c_void_p else e for e in v]
        out.append((name, v))
    return out


def field_text(v, addr):
    if isinstance(v, torch.Tensor):
        if v.dtype == torch.int32:
            return ("i32", tuple(v.shape), v.cpu().flatten().tolist())
        if v.dtype == torch.uint8:
            return ("u8", v.numel())
        return ("t", addr(v.data_ptr()), tuple(v.shape), tuple(v.stride()))
    if isinstance(v, (list, tuple)):
        return [field_text(e, addr) for e in v]
    return v


def plan_text(voc, p, key):
    addr = Addresses(vars(voc), p)
    lines = [repr(("plan", key, p["B"], p["N"], p["L"], field_text(p["mel_in"], addr), field_text(p["wav"], addr)))]
    for s, (pos, structs) in zip(p["steps"], p["meta"]):
        lines.append(repr((pos, field_text(tuple(s), addr), [struct_text(g, addr) for g in structs] if structs else None)))
    lines.append(repr(("totals", p["conv_launches"], p["act_bytes"], p["n_act"], p["conv_executed_flops"], p["conv_direct_flops"],
                       "cache bytes", voc._plans._bytes[key])))
    return lines, addr.unknown


def ragged_text(voc, rp):
    key = ("ragged",) + tuple(rp["frames"])
    addr = Addresses(vars(voc), rp)
    raw = rp["desc"].cpu().numpy().tobytes()
    lines = [repr(("ragged plan", key, len(raw), [(sp["B"], sp["N"], field_text(sp["wav"], addr)) for sp in rp["subs"]]))]
    for s in rp["steps"]:
        row = [field_text(tuple(s), addr)]
        if s[0] in RAGGED_DESC:
            typ, second = RAGGED_DESC[s[0]]
            row.append([struct_text(g, addr) for g in (typ * s[2]).from_buffer_copy(raw, s[1])])
            if second:
                off, n, elem = second
                row.append([e if isinstance(e, int) else list(e) for e in (elem * s[n]).from_buffer_copy(raw, s[off])])
        lines.append(repr(tuple(row)))
    lines.append(repr(("cache bytes", voc._ragged._bytes[key])))
    return lines, addr.unknown


def model_text(cfgname, form, env=None):
    """All plans of the grid for one model; env: switches set while the model is built (they are read once, then)."""
    cfg = getattr(synth, cfgname)
    old = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    try:
        voc = Vocoder(cfg, synth.make_vocoder_state_dict(cfg, 1), "cpu", conv_form=form)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    lines, unknown = [f"== {cfgname} {form} {sorted((env or {}).items())}"], 0
    plans = [((b, n), dict()) for b, n in SHAPES]
    if cfgname == "SYNTH_CFG" and not env:
        plans += [((1, 400), dict(ref_frames=2000)), ((1, 50), dict(inst=1))]
    for (b, n), kw in plans:
        p = voc.plan(b, n, **kw)
        key = next(k for k, v in voc._plans.items() if v is p)
        text, u = plan_text(voc, p, key)
        lines += text
        unknown += u
    if cfgname == "SYNTH_CFG" and not env and form != "direct":
        for frames in RAGGED:
            text, u = ragged_text(voc, voc.plan_ragged(frames))
            lines += text
            unknown += u
    return lines, unknown


def dump_all():
    lines, unknown = [], 0
    jobs = [(c, f, None) for c in CONFIGS for f in FORMS]
    jobs += [("SYNTH_CFG", f, {sw: "0"}) for sw in ("FH_WINO_SPLITK", "FH_UPS_FUSE") for f in FORMS]
    for job in jobs:
        text, u = model_text(*job)
        lines += text
        unknown += u
    return "\n".join(lines) + "\n", unknown


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", help="write the canonical text to this file")
    args = ap.parse_args()
    text, unknown = dump_all()
    if args.out:
        Path(args.out).write_text(text)
    print(f"sha256 {hashlib.sha256(text.encode()).hexdigest()}  lines {text.count(chr(10))}  UNKNOWN addresses {unknown}")
    sys.exit(1 if unknown else 0)
