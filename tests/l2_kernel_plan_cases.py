"""The recorder behind tests/golden/l2_kernel_plan_cases.json: what the library's host-side queries of the level-2 family answer over
a grid of shapes, sizes at every limit, relation counts at every LDS edge, and switch settings.  No GPU is touched: the queries are
mvin_gather_attn_l2_supported / _enc_supported / _variant_ex / _prj_supported / _agg_supported, mvin_score_l2_folded_supported /
_folded_gather_supported and ops.gather_attn_l2_wpp_supported.  The library reads a switch once per process, so every switch setting
is answered by a child process of its own.

    python tests/l2_kernel_plan_cases.py --write tests/golden/l2_kernel_plan_cases.json [--root TREE]

writes the file from the library built in TREE (default: this checkout); tests/test_l2_kernel_plan_host.py compares the committed file
with the answers of the library under test.  The file was written from the commit before mvin_l2_kernel_plan.h existed and again from
the one that introduced it: byte-equal.

The edges are found here by loops over formulas written out in this file (an independent statement of them, like wpp_lds_limit_nr of
tests/test_gpu_l2_f64.py), not read from the library."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "l2_kernel_plan_cases.json")
DIMS = (16, 32, 64, 128)
FANS = (4, 8, 16, 32, 64, 128, 256)
# unset, and every switch a query can show (MVIN_L2_D32ENC shows in none: recorded to say so)
SETTINGS = ("", "MVIN_L2_D16=0", "MVIN_L2_D32=0", "MVIN_L2_D32ENC=0", "MVIN_L2_SPLIT=0", "MVIN_L2_WPP=0", "MVIN_L2_AGG=0", "MVIN_L2_FOLD_GATHER=0")


def ru4(n):
    return (n + 3) & ~3


# dynamic LDS in bytes, per kernel, as functions of (nR, K): written out from the kernels' layouts
LDS = {
    "d16": (lambda nR, K: (2 * ru4(nR) + 4 * (3 * 16 * 20 + 32)) * 4, 64 * 1024),
    "d32": (lambda nR, K: (2 * ru4(nR) + 3 * 32 * 32 + 4 * (2 * 16 * 36 + 32 + 2 * 16 * K + 96)) * 4, 64 * 1024),
    "wpp": (lambda nR, K: (2 * ru4(nR) + 4 * (16 * 132 + 4 * 2 * (K + 4))) * 4, 48 * 1024),
    "agg": (lambda nR, K: (ru4(nR) + 4 * (16 * 132 + 4 * 2 * (K + 4))) * 4, 48 * 1024),
    "fold32": (lambda nR, K: (ru4(nR) + 4 * (16 * 68 + 8 * 2 * (K + 4))) * 4, 48 * 1024),
}


def last_nr_inside(kernel, K):
    """The last relation count whose launch stays inside the kernel's LDS budget (None: every count up to 4096 does)."""
    size, budget = LDS[kernel]
    nR = 0
    while size(nR + 1, K) <= budget:
        nR += 1
        if nR > 4096:
            return None
    return nR


def relation_counts(kernel=None, K=0):
    out = [0, 1, 9, 4096, 4097]
    edge = last_nr_inside(kernel, K) if kernel else None
    if edge is not None:
        out += [edge - 1, edge, edge + 1, edge + 2]
    return sorted(set(n for n in out if n >= 0))


def around(limit_bytes, row_bytes):
    """Row counts at a byte limit `rows * row_bytes < limit_bytes`: the last admitted one and one more (where an int holds them)."""
    last = (limit_bytes - 1) // row_bytes
    return [n for n in (last, last + 1) if 0 < n < 2 ** 31]


def entity_counts(D, K, elem=4):
    """1000, and every byte / count limit of the family at its last admitted entity count and one more."""
    out = {0, 1000}
    for limit, row in ((2 ** 31, K * 4), (2 ** 32, D * elem), (2 ** 32 - 4096, D * elem), (2 ** 30, D * 4)):
        out.update(around(limit, row))
    out.update((2 ** 24, 2 ** 24 + 1))
    return sorted(out)


def grid():
    cases = []
    for D in (8,) + DIMS + (256,):
        for K in (2, 3) + FANS + (12, 512):
            cases.append(("supported", D, K))
            cases.append(("enc_supported", D, K))
            cases.append(("wpp_supported", D, K))
    for D in DIMS:
        for K in FANS:
            for probs in (0, 1):
                for bf16 in (0, 1):
                    cases.append(("variant", D, K, 100, 1000, probs, bf16))
    # the variant query at its byte limits: the shapes of the four kernels it can name, and one it cannot
    for D, K in ((16, 4), (16, 16), (32, 8), (32, 16), (32, 32), (64, 32), (128, 128), (64, 8)):
        for bf16 in (0, 1):
            for nE in entity_counts(D, K, 2 if bf16 else 4):
                cases.append(("variant", D, K, 100, nE, 0, bf16))
            for P in [0, 1] + around(2 ** 31, D * 4):
                cases.append(("variant", D, K, P, 1000, 0, bf16))
    for D in DIMS:
        for K in FANS:
            for enc in (0, 1):
                kernel = "d32" if (D == 32 and K in (8, 16)) else None
                for nR in relation_counts(kernel, K):
                    cases.append(("prj_supported", D, K, enc, 1000, nR))
    for D, K in ((32, 8), (32, 16), (32, 32), (64, 16), (64, 128), (128, 32)):
        for enc in (0, 1):
            for nE in entity_counts(D, K):
                cases.append(("prj_supported", D, K, enc, nE, 9))
    for D in DIMS:
        for K in (8, 16, 32, 64, 128):
            for query, kernel in (("agg_supported", "agg"), ("folded_supported", "fold32" if D == 32 else "agg"), ("folded_gather_supported", "wpp")):
                for nR in relation_counts(kernel, K):
                    cases.append((query, D, K, 1000, nR))
    for D, K in ((64, 16), (64, 64), (32, 16), (32, 32), (64, 32)):
        for query in ("agg_supported", "folded_supported", "folded_gather_supported"):
            for nE in entity_counts(D, K):
                cases.append((query, D, K, nE, 9))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def answers(cases):
    """One digit per case from the library of this process (its switches are whatever the environment says)."""
    from mvin_amd import _lib, ops
    lib = _lib.load()
    ask = {
        "supported": lib.mvin_gather_attn_l2_supported,
        "enc_supported": lib.mvin_gather_attn_l2_enc_supported,
        "variant": lib.mvin_gather_attn_l2_variant_ex,
        "prj_supported": lib.mvin_gather_attn_l2_prj_supported,
        "agg_supported": lib.mvin_gather_attn_l2_agg_supported,
        "folded_supported": lib.mvin_score_l2_folded_supported,
        "folded_gather_supported": lib.mvin_score_l2_folded_gather_supported,
        "wpp_supported": lambda D, K: int(ops.gather_attn_l2_wpp_supported(D, K)),
    }
    return "".join(str(int(ask[c[0]](*c[1:]))) for c in cases)


def record(root=ROOT, cases=None, settings=SETTINGS):
    """{setting: digits}: one child process per switch setting (four at a time), each running this file against the tree at `root`."""
    cases = grid() if cases is None else cases
    out, pending = {}, list(settings)
    while pending:
        batch, pending = pending[:4], pending[4:]
        procs = []
        for s in batch:
            env = {k: v for k, v in os.environ.items() if not k.startswith("MVIN_L2_")}
            env["PYTHONPATH"] = root
            if s:
                name, value = s.split("=")
                env[name] = value
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=root, stdin=subprocess.PIPE,
                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        for s, p in zip(batch, procs):
            so, se = p.communicate(json.dumps(cases), timeout=300)
            assert p.returncode == 0, (s, se[-2000:])
            out[s] = so.strip().splitlines()[-1]
            assert len(out[s]) == len(cases), (s, len(out[s]))
    return out


def pack(cases, recorded):
    """The file's content: the cases, the answers with every switch unset, and per switch setting the cases it changes."""
    base = recorded[""]
    doc = {"cases": [list(c) for c in cases], "unset": base, "switches": {}}
    for s, digits in recorded.items():
        if s:
            doc["switches"][s] = {str(i): int(d) for i, (d, b) in enumerate(zip(digits, base)) if d != b}
    return doc


def dumps(doc):
    lines = ["{", '"cases": [']
    rows = [json.dumps(c, separators=(",", ":")) for c in doc["cases"]]
    for i in range(0, len(rows), 8):
        lines.append(",".join(rows[i:i + 8]) + ("," if i + 8 < len(rows) else ""))
    lines += ["],", '"unset": ' + json.dumps(doc["unset"]) + ",", '"switches": ' + json.dumps(doc["switches"], sort_keys=True), "}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if "--child" in sys.argv:
        print(answers([tuple(c) for c in json.loads(sys.stdin.read())]))
    else:
        root = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else ROOT
        path = sys.argv[sys.argv.index("--write") + 1]
        cases = grid()
        doc = pack(cases, record(root, cases))
        with open(path, "w") as f:
            f.write(dumps(doc))
        changed = {s: len(v) for s, v in doc["switches"].items()}
        print(f"{len(cases)} cases, outcomes with every switch unset: { {d: doc['unset'].count(d) for d in sorted(set(doc['unset']))} }, changed per switch: {changed}")
