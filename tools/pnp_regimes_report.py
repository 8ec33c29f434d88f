"""Classification counts of every form of the pose solver over the regimes of tests/test_pnp_regimes_host.py, as the markdown table of
profiles/pnp_regimes.md.

    python tools/pnp_regimes_report.py [--gpu] [--seeds 1 2 3 ...]

Without --gpu: the four host forms.  With --gpu: the device forms of tests/test_gpu_pnp_regimes.py as well (one process, one visit).
--seeds: classify these seeds of EVERY regime instead of the table's own (a wider look than the tests take; host forms only)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--seeds", type=int, nargs="*", default=None)
    a = ap.parse_args()
    import test_pnp_regimes_host as T
    from boxdreamer_amd import pnp
    pnp._HAVE_CV2 = False
    cases = T.ALL_CASES if a.seeds is None else [(k, s) for k in T.REGIMES for s in a.seeds]
    rows = {}
    for name, seed in cases:
        for form, (c, poses, cls) in T.host_results(name, seed).items():
            rows[(name, seed, "host " + form)] = T.counts(cls)
        if a.gpu and a.seeds is None:
            import test_gpu_pnp_regimes as G
            for form, (c, poses, cls, rms) in G.device_results(name, seed).items():
                rows[(name, seed, "device " + form)] = T.counts(cls)
    forms = sorted({k[2] for k in rows}, key=lambda f: (f.startswith("device"), f))
    short = {"at_reference": "ref", "other_minimum": "other", "failed": "failed", "behind": "behind", "not_stationary": "not stat."}
    print("| regime | seed | " + " | ".join(forms) + " |")
    print("|---|---|" + "---|" * len(forms))
    for name, seed in cases:
        cells = []
        for f in forms:
            k = rows.get((name, seed, f))
            cells.append("-" if k is None else ", ".join(f"{v} {short[x]}" for x, v in k.items() if v))
        print(f"| {name} | {seed} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
