"""Developer aid (GPU box): the bench line of several libraries under variants/ alternated inside one job, then the fluxes of
bench.py --dump-outputs per library compared byte for byte with the first one's (profiles/flux_chain_ab.txt).
    profiles/build_variant.sh parent   (on the parent commit)        profiles/build_variant.sh sp -DVAG_FLUX_CHAIN=1   ...
    python profiles/flux_chain_ab.py parent,sp,... [ROUNDS [SECONDS]]   -> $OUT/ab_chain.txt (OUT: run_out/ by default)
The first name is the reference.  No new round starts after SECONDS; the job stops at the first run that does not exit 0."""
import json, os, subprocess, sys, time, filecmp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("OUT") or os.path.join(ROOT, "run_out")
os.makedirs(OUT, exist_ok=True)
names = sys.argv[1].split(",")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
log = open(os.path.join(OUT, "ab_chain.txt"), "a")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n"); log.flush()


def run(cmd, lib, limit):
    env = dict(os.environ, VAG_LIB_PATH=os.path.join(ROOT, "variants", "libvag_%s.so" % lib))
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        say("STOP: %s with %s exit %d after %.0f s\n%s\n%s" % (cmd, lib, p.returncode, time.time() - t0, p.stdout[-2000:], p.stderr[-3000:]))
        sys.exit(1)
    return p.stdout


budget = float(sys.argv[3]) if len(sys.argv) > 3 else 1e9  # seconds for the rounds: no new round starts after it
t_start = time.time()
ms = {n: [] for n in names}
for r in range(rounds):
    if time.time() - t_start > budget:
        say("budget reached after %d rounds" % r)
        break
    for n in names:
        out = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], n, 240)
        d = json.loads(out.strip().splitlines()[-1])
        ms[n].append(d["ms_per_step"])
        say("round %d %-8s %.4f ms  stages %s" % (r, n, d["ms_per_step"], d.get("stage_ms")))
import statistics
base = statistics.median(ms[names[0]])
for n in names:
    v = ms[n]
    say("== %-8s median %.4f  spread %.4f  min %.4f  vs %s %+.2f %%   %s" % (n, statistics.median(v), max(v) - min(v), min(v), names[0],
                                                                          100 * (statistics.median(v) / base - 1), [round(x, 4) for x in v]))
for n in names:
    d = os.path.join(OUT, "dump_" + n)
    run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", d], n, 240)
    same = filecmp.cmp(os.path.join(d, "flux_density.npy"), os.path.join(OUT, "dump_" + names[0], "flux_density.npy"), shallow=False)
    say("dump %-8s flux_density.npy byte-equal to %s: %s" % (n, names[0], same))
    if n != names[0]:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
for f in os.listdir(os.path.join(OUT, "dump_" + names[0])):
    os.remove(os.path.join(OUT, "dump_" + names[0], f))
