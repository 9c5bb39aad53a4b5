"""The ODE methods of the sampler beside each other on BASELINE configs[1] (B = 1, one 10 s clip, 12 -> 48 kHz, full-width vocoder).
    python tools/ode_bench.py [--parent DIR] [out.md]
For each method of flowhigh_amd.ode.ODE_METHODS at timestep 1 and 2: ms per generate_from_device call (device-resident input, as
bench.py times it) and the library's launches per call.  --parent DIR: a source tree of the parent commit with its library built
in it (tools/build_prev.sh makes the library; `git archive <rev> flowhigh_amd | tar -x -C DIR` the tree): its euler x 1 and
midpoint x 1 are measured in the same session, once before and once after this build's rows.

Method: every build is measured in a process of its own (a fresh child of this script, which never opens the GPU itself), its
entries alternating in that process; after a warm-up of every entry, SAMPLES samples of each, a sample = device events around
enough calls to last at least MIN_SAMPLE_S, ended by a synchronise; per entry the median and the spread (max - min).
Launches: calls of the library's enqueueing C entries (fh_*_f32 taking a stream; one kernel launch each) during one call,
counted by a proxy around the loaded library -- torch's own copies and fills are not in the count.
These numbers are records, not thresholds.  profiles/ode_methods.md holds a run."""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SECS, SR_IN = 10.0, 12000
MIN_SAMPLE_S = 0.3
SAMPLES = 5
CHILD_TIMEOUT_S = 420


def child(root, entries):
    """Measure `entries` = [(method, timestep)] with the package found under `root`; prints one JSON line."""
    sys.path.insert(0, str(root))
    import torch
    from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth
    from flowhigh_amd.planner import resolve_conv_form
    dev = torch.device("cuda:0")
    cfg = synth.SYNTH_CFG
    form = resolve_conv_form()[0]
    fh = FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev, conv_form=form)
    n_frames = int(SECS * 100)
    x = torch.from_numpy(synth.lowres_clip(0, SECS, SR_IN))[None].to(dev)
    z = synth.prior_noise(0, n_frames).to(dev).contiguous()
    models = {m: FlowHighSR(fh, torchdiffeq_ode_method=m, upsampling_method="hip") for m in {m for m, _ in entries}}
    runs = {(m, k): (lambda m=m, k=k: models[m].generate_from_device(x, SR_IN, k, noise=z)) for m, k in entries}

    def timed(run, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    reps = {}
    for key, run in runs.items():                   # warm-up of every shape and plan, then the size of a sample
        for _ in range(3):
            run()
        reps[key] = max(2, int(MIN_SAMPLE_S * 1e3 / timed(run, 3)) + 1)
    ms = {key: [] for key in runs}
    for _ in range(SAMPLES):
        for key, run in runs.items():
            ms[key].append(timed(run, reps[key]))

    class Counting:
        """The loaded library with its enqueueing entries counted."""
        def __init__(self, lib):
            self.lib, self.n = lib, 0

        def __getattr__(self, name):
            fn = getattr(self.lib, name)
            sig = hip._SIGS.get(name)
            if not (name.endswith("_f32") and sig and sig[-1] is hip._P):
                return fn

            def counted(*args):
                self.n += 1
                return fn(*args)
            return counted
    real = hip.lib()
    proxy = Counting(real)
    hip._lib = proxy
    launches = {}
    for key, run in runs.items():
        proxy.n = 0
        run()
        launches[key] = proxy.n
    hip._lib = real
    torch.cuda.synchronize()
    rows = [dict(method=m, timestep=k, ms=sorted(ms[m, k])[SAMPLES // 2], spread_ms=max(ms[m, k]) - min(ms[m, k]),
                 calls_per_sample=reps[m, k], launches=launches[m, k]) for m, k in entries]
    print("ODE_BENCH " + json.dumps(dict(conv_form=form, device=torch.cuda.get_device_name(0), rows=rows)), flush=True)


def run_child(root, entries):
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", str(root), json.dumps(entries)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ODE_BENCH ")]
    if r.returncode != 0 or not lines:
        raise SystemExit(f"ode_bench: the measurement in {root} ended with {r.returncode}:\n{r.stderr[-3000:]}")
    print(f"measured {len(entries)} entries in {root}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len("ODE_BENCH "):])


def main(argv):
    parent = None
    if "--parent" in argv:
        i = argv.index("--parent")
        parent = Path(argv[i + 1]).resolve()
        argv = argv[:i] + argv[i + 2:]
    out_path = argv[0] if argv else None
    sys.path.insert(0, str(ROOT))
    from flowhigh_amd import ode                     # (no GPU import)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    old = [("euler", 1), ("midpoint", 1)]
    before = run_child(parent, old) if parent else None
    here = run_child(ROOT, [(m, k) for k in (1, 2) for m in ode.ODE_METHODS])
    after = run_child(parent, old) if parent else None
    say(f"BASELINE configs[1]: B = 1, one {SECS:g} s clip, {SR_IN} -> 48000 Hz, conv_form '{here['conv_form']}', {here['device']}; "
        f"median of {SAMPLES} samples of >= {MIN_SAMPLE_S} s, spread = max - min")
    say()
    say("| build | method x timestep | field evaluations | ms per call | spread ms | calls per sample | launches per call |")
    say("|---|---|---|---|---|---|---|")

    def table(name, res):
        for r in res["rows"]:
            say(f"| {name} | {r['method']} x {r['timestep']} | {ode.evaluations(r['method'], r['timestep'])} | {r['ms']:.3f} | "
                f"{r['spread_ms']:.3f} | {r['calls_per_sample']} | {r['launches']} |")
    if before:
        table("parent commit, before", before)
    table("this build", here)
    if after:
        table("parent commit, after", after)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(Path(sys.argv[2]), [tuple(e) for e in json.loads(sys.argv[3])])
    else:
        main(sys.argv[1:])
