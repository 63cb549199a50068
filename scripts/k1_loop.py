"""K1's whole window loop, classified like scripts/k1_isa.py's hot path.

k1_isa.hot_path spans the hashing of one window (first table read to last);
the per-window work around it (the window's place in its run, its word loads,
funnel shifts and reverse complements, the loop bookkeeping) lies outside that
span.  This counts the loop that contains the hash body from its head to its
back edge, skipping the bodies of forward s_cbranch_execz branches (the
candidate pushes, the drain, the other-run path), and prices the classes at
the costs of profiles/r04_k1_issue_model.json.  Also prints the kernel's
register counts from the code object's metadata.

Usage: python scripts/k1_loop.py [lib.so ...]
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import k1_isa  # noqa: E402

READELF = os.path.join(os.path.dirname(k1_isa.OBJDUMP), "llvm-readelf")
META = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")


def class_costs():
    with open(os.path.join(ROOT, "profiles", "r04_k1_issue_model.json")) as f:
        return json.load(f)["class_cost_cycles"]


def kernel_meta(lib_path, symbol=k1_isa.K1_SYMBOL):
    """{field: value} of the kernel's metadata note in the gfx950 code object."""
    tmp = tempfile.mkdtemp(prefix="k1loop")
    try:
        lib = os.path.join(tmp, "lib.so")
        shutil.copy(lib_path, lib)
        subprocess.run([k1_isa.OBJDUMP, "--offloading", lib], cwd=tmp, capture_output=True, timeout=120)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            txt = subprocess.run([READELF, "--notes", os.path.join(tmp, f)], capture_output=True, text=True,
                                 timeout=120).stdout
            for block in re.split(r"\n\s*- \.agpr_count:", txt):
                if re.search(r"\.name:\s*\S*%s" % re.escape(symbol), block):
                    out = {"agpr_count": block.split("\n")[0].strip()}
                    for k in META:
                        m = re.search(r"\.%s:\s*(\S+)" % k, block)
                        if m:
                            out[k] = m.group(1)
                    return out
        return {}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def window_loop(listing_addr):
    """[(mnemonic, operands)] of the innermost loop around the hash body on
    its no-candidate path."""
    base = listing_addr[0][0]
    reads = [i for i, x in enumerate(listing_addr) if x[1] == "ds_read_b128"]
    lo, hi = reads[0], reads[-1]
    best = None
    for i, (addr, mn, _ops, tgt) in enumerate(listing_addr):
        if i > hi and (mn.startswith("s_cbranch") or mn == "s_branch") and tgt is not None and tgt + base < addr:
            ti = next(j for j, x in enumerate(listing_addr) if x[0] >= tgt + base)
            if ti <= lo and (best is None or i - ti < best[1] - best[0]):
                best = (ti, i)
    if best is None:
        return []
    out, i = [], best[0]
    while i <= best[1]:
        addr, mn, ops, tgt = listing_addr[i]
        if mn == "s_cbranch_execz" and tgt is not None and tgt + base > addr:
            j = i + 1
            while j < len(listing_addr) and listing_addr[j][0] < tgt + base:
                j += 1
            # (the loop's own guard spans the hash body: not a side branch)
            if not any(listing_addr[x][1] == "ds_read_b128" for x in range(i, j)):
                i = j
                continue
        out.append((mn, ops))
        i += 1
    return out


def report(lib):
    cost = class_costs()
    seg = 44.0  # k-mers per window at k = 21
    listing = k1_isa.kernel_listing(lib, with_addr=True)
    print(lib)
    print("  fingerprint", k1_isa.fingerprint([(x[1], x[2]) for x in listing]), kernel_meta(lib))
    for name, path in (("hot path", k1_isa.hot_path(listing)), ("window loop", window_loop(listing))):
        h = k1_isa.histogram(path)
        nv = h["dual"] + h["full"] + h["wide"]
        print("  %-11s %s: %d VALU (%.2f per k-mer), %.2f cycles per k-mer" %
              (name, h, nv, nv / seg, sum(h[k] * cost[k] for k in cost) / seg))


if __name__ == "__main__":
    for lib in sys.argv[1:] or [os.path.join(ROOT, "galah_amd", "lib", "libgalahgpu.so")]:
        report(lib)
