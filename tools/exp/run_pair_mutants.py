"""Run every pair / split mutant of tools/exp/make_pair_mutants.py against the bf16 x 6 tests, one process at a time, each under its
own time limit, and write the table mutant x {tests/test_hip_bf16x6_pairs.py, the kernel's earlier bf16 x 6 tests}: killed or
survived.  A mutant counts as killed only by assertion failures (a mismatch); anything else -- a crash, a time-out, a HIP or
Python error, a fuzz subprocess that did not end normally -- stops the run there (the table then says so).
    python tools/exp/run_pair_mutants.py [--out FILE] [kernel ...]      (kernel: gemm narrow w43 w54 attn_qk attn_pv; default: the first four)
The attention kernel's mutants (attn_qk, attn_pv) run against tests/test_hip_attention_bf.py: new = its pair pins (-k pairs),
existing = its random-input accuracy tests (RMS error to float64 against the fp32 kernel's); their table is
profiles/attention_bf16x6.md's, so give them an --out of their own.
The table (default profiles/r07_bf16x6_pair_mutants.txt) is written anew on every run; the report of a test set that stopped the
run goes beside it, <mutant>.stop.log."""
import os
import re
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tools" / "exp"))
from make_pair_mutants import LIB_DIR, MUTANTS      # noqa: E402

PAIR_FILE = "tests/test_hip_bf16x6_pairs.py"
ATTN_FILE = "tests/test_hip_attention_bf.py"
NEW = {"gemm": [PAIR_FILE, "-k", "gemm_bf16x6"], "narrow": [PAIR_FILE, "-k", "narrow_bf16x6"], "w43": [PAIR_FILE, "-k", "wino43_bf16x6"],
       "w54": [PAIR_FILE, "-k", "wino54_bf16x6"], "attn_qk": [ATTN_FILE, "-k", "pairs"], "attn_pv": [ATTN_FILE, "-k", "pairs"]}
DEFAULT_KERNELS = ["gemm", "narrow", "w43", "w54"]
OLD = {"gemm": ["tests/test_hip_ops.py::test_gemm_linear", "tests/test_hip_ops.py::test_gemm_geglu_packed", "-k", "bf16x6"],
       "narrow": ["tests/test_hip_amp.py::test_amp_conv_only", "tests/test_hip_amp.py::test_narrow_kernels_randomised_configurations",
                  "-k", "direct"],
       "w43": ["tests/test_hip_ops.py::test_conv_wino_bf16x6_fuzz"],
       "w54": ["tests/test_hip_ops.py::test_conv_wino54_bf16x6_fuzz",
               "tests/test_hip_ops.py::test_conv_wino54_bf16x6_tile_heights_give_the_same_bits_and_the_fp32_forms_values"],
       "attn_qk": [ATTN_FILE, "-k", "rms_error"], "attn_pv": [ATTN_FILE, "-k", "rms_error"]}
LIMIT = {"new": 240, "old": 900}
# a failure whose report says any of these is not a mismatch: the GPU or the process went wrong (the fuzz tests run a subprocess
# and quote its stderr: a Python exception there shows its traceback, a signal a negative returncode; narrow_fuzz.py's own
# exit status 1 on mismatches is a mismatch)
FAULT = re.compile(r"HipError|hipError|HIP error|RuntimeError|Memory access fault|illegal|core dumped|Aborted|Segmentation|"
                   r"Traceback|TimeoutExpired|returncode=-\d")
MISMATCH = ("Failed:", "AssertionError", "assert ")      # pytest.fail (the new module) and assert statements
SECTION = re.compile(r"^_+ \S.* _+$")                   # a failure's report header (one underscore a side for a long test id)


def classify(rc, out):
    """(verdict, first failure) of one pytest process (-q -rfE --tb=short): survived | killed | STOP ...  Killed: every failure's
    report (the section under its ___ header) opens with a mismatch and no report line names a fault."""
    lines = out.splitlines()
    tail = ([ln for ln in lines if ln.strip()] or [""])[-1]
    if rc == 0:
        return "survived", tail
    sections, cur = [], None
    for ln in lines:
        if SECTION.match(ln):
            cur = []
            sections.append(cur)
        elif cur is not None and ln.startswith("E "):
            cur.append(ln[1:].strip())
    n_failed = sum(ln.startswith("FAILED ") for ln in lines)
    errors = [ln for ln in lines if ln.startswith("ERROR ")]
    faults = [e for s in sections for e in s if FAULT.search(e)]
    firsts = [s[0] if s else "" for s in sections]
    if (rc == 1 and n_failed and n_failed == len(sections) and not errors and not faults
            and all(f.startswith(MISMATCH) for f in firsts)):
        return "killed", firsts[0]
    why = faults[0] if faults else errors[0] if errors else next((f for f in firsts if not f.startswith(MISMATCH)), tail)
    return f"STOP rc={rc}", why or tail


def pytest(lib, args, limit, log):
    env = dict(os.environ, FH_LIB_PATH=str(lib))
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", "-q", "-rfE", "--tb=short", "-m", "gpu",
                        "-p", "no:cacheprovider", *args], cwd=ROOT, env=env, capture_output=True, text=True)
    verdict, why = classify(p.returncode, p.stdout + "\n" + p.stderr)
    if verdict.startswith("STOP"):                             # (the whole report, for the reader of the table)
        log.write_text(p.stdout + "\n" + p.stderr)
    return verdict, why[:200], time.time() - t0


def main():
    args = sys.argv[1:]
    out = ROOT / "profiles" / "r07_bf16x6_pair_mutants.txt"
    if "--out" in args:
        i = args.index("--out")
        out = Path(args[i + 1])
        del args[i:i + 2]
    kernels = args or DEFAULT_KERNELS
    rows, stop = [], False
    for name, kernel, _, _ in MUTANTS:
        if kernel not in kernels or stop:
            continue
        lib = LIB_DIR / f"{name}.so"
        if not lib.exists():
            rows.append((name, ("not built", "make_pair_mutants.py did not build it", 0.0), ("not built", "", 0.0)))
            continue
        log = out.parent / f"{name}.stop.log"
        r_new = pytest(lib, ["-x", *NEW[kernel]], LIMIT["new"], log)
        stop = r_new[0].startswith("STOP")
        r_old = ("not run", "", 0.0) if stop else pytest(lib, OLD[kernel], LIMIT["old"], log)
        stop = stop or r_old[0].startswith("STOP")
        rows.append((name, r_new, r_old))
        print(f"{name:20s} new: {r_new[0]:9s} ({r_new[2]:5.1f} s)  existing: {r_old[0]:9s} ({r_old[2]:5.1f} s)  {r_new[1][:90]}", flush=True)
        if stop:
            print(f"  stopped: {(r_new if r_new[0].startswith('STOP') else r_old)[1]}", flush=True)
    with open(out, "w") as f:
        f.write("# bf16 x 6 pair / split mutants (tools/exp/make_pair_mutants.py), one pytest process per mutant and test set\n"
                "# (tools/exp/run_pair_mutants.py).  new = the kernel's pair pins; existing = its other bf16 x 6 tests:\n")
        for k in kernels:
            f.write(f"#   {k}: new = {' '.join(NEW[k])}; existing = {' '.join(OLD[k])}\n")
        f.write("# killed = a test failed on an assertion (the new module: an exact torch.equal mismatch, its first failure below);\n"
                "# survived = every test passed.\n")
        f.write(f"{'mutant':20s} {'new':10s} {'existing':10s} first failure of the new module\n")
        for name, r_new, r_old in rows:
            f.write(f"{name:20s} {r_new[0]:10s} {r_old[0]:10s} {r_new[1]}\n")
        if stop:
            last = rows[-1]
            f.write(f"stopped after {last[0]}: {(last[1] if last[1][0].startswith('STOP') else last[2])[1]}\n")
    return 1 if stop else 0


if __name__ == "__main__":
    sys.exit(main())
