"""Compare the gfx950 kernels of two builds of the library, no GPU needed:
  python tools/compare_kernels.py OLD/libdsptoolbox_amd.so NEW/libdsptoolbox_amd.so
Per-kernel machine-code fingerprints (_build.kernel_fingerprints) and, where a kernel_resources.json lies beside each
library, registers / scratch / LDS.  Exit status 1 when a kernel was added, removed or changed."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dsptoolbox_amd import _build  # noqa: E402


def load(lib):
    res_path = os.path.join(os.path.dirname(lib), "kernel_resources.json")
    res = json.load(open(res_path)) if os.path.exists(res_path) else {}
    return _build.kernel_fingerprints(lib), res


def main(old_lib, new_lib):
    (old, old_res), (new, new_res) = load(old_lib), load(new_lib)
    keys = ("vgpr", "agpr", "sgpr", "scratch", "lds", "occupancy")
    fig = lambda res, k: " ".join("%s=%s" % (f, res.get(k, {}).get(f, "?")) for f in keys)
    print("compiler:", _build._run_compiler_id())
    print("flags:", " ".join(_build.FLAGS))
    print("kernels: old %d, new %d" % (len(old), len(new)))
    print("only in old:", sorted(set(old) - set(new)) or "none")
    print("only in new:", sorted(set(new) - set(old)) or "none")
    changed = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    moved = sorted(k for k in set(old) & set(new) if old_res.get(k) != new_res.get(k))
    print("same name, same machine code: %d" % (len(set(old) & set(new)) - len(changed)))
    print("same name, other machine code: %d" % len(changed))
    for k in changed:
        print("  %s\n    old %s  %s\n    new %s  %s" % (k, old[k], fig(old_res, k), new[k], fig(new_res, k)))
    print("same name, other resource figures: %d" % len(moved))
    for k in moved:
        print("  %s\n    old %s\n    new %s" % (k, fig(old_res, k), fig(new_res, k)))
    return 1 if changed or moved or set(old) != set(new) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
