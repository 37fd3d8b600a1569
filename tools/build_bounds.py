"""Debug build of the HIP library with -DCAR_BOUNDS (csrc/car_common.h): every LDS-DMA / buffer-load / row-load helper of the kernels
compares the range it is about to read with the extent its launcher passed and TRAPS outside it.  Never part of the product
(``__graft_entry__.build()`` does not know this file).  Output: tools/_dev/libcar_bounds.so — run the out-of-bounds harness on it with
CAR_OOB_FULL_LIB=tools/_dev/libcar_bounds.so python tests/oob_runner.py <family>   (tools/oob_selfcheck.sh does all of it).
``--reintroduce-0d74f26``: also tools/_dev/liboldlin16_bounds.so — today's car_linear16.hip and car_row_sweep.h with the bug commit 0d74f26 fixed put back
(three LDS-DMA pieces issued whatever the column group's width: a narrow group's third piece copies from behind its chunk)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = os.path.join(ROOT, "tools", "_dev")


def build(reintroduce: bool = False):
    import __graft_entry__ as ge
    os.makedirs(os.path.join(DEV, "bounds_obj"), exist_ok=True)
    headers = [os.path.join(ge.CSRC, f) for f in os.listdir(ge.CSRC) if f.endswith(".h")] + [os.path.join(ROOT, "include", f) for f in ("car_hip.h", "car_match.h", "car_encoder.h", "car_trunk.h", "car_decoder.h")]
    objs, procs = [], []
    for unit, extra in ge.UNITS.items():
        src, obj = os.path.join(ge.CSRC, unit), os.path.join(DEV, "bounds_obj", unit.replace(".hip", ".o"))
        objs.append(obj)
        if ge._stale(obj, [src, *headers, os.path.abspath(__file__)]):
            procs.append(subprocess.Popen([ge._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DCAR_BOUNDS", "-c", src, "-o", obj,
                                           "-I", os.path.join(ROOT, "include"), "-I", ge.CSRC, *extra]))
    if any(p.wait() != 0 for p in procs):
        sys.exit("build_bounds: hipcc failed")
    lib = os.path.join(DEV, "libcar_bounds.so")
    if ge._stale(lib, objs):
        subprocess.check_call([ge._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs])
    out = [lib]
    if reintroduce:
        # the lines this tool puts back stand in car_linear16.hip (the issue of chunk 0) and in car_row_sweep.h (the static_assert, which
        # would refuse them): patched copies of both, the header BESIDE the unit (a quoted include resolves beside the including
        # file first), every other header from csrc/ as usual
        rep = (("p < pieces_of(NT); ++p", "p < kPieces; ++p"),
               ('static_assert(kWaves * pieces_of(NT) <= 3 * 2 * NT,', 'static_assert(true || kWaves * pieces_of(NT) <= 3 * 2 * NT,'))
        srcf = os.path.join(DEV, "linear16_with_0d74f26_reverted.hip")
        for name, out_path, need in (("car_linear16.hip", srcf, "p < kPieces; ++p"), ("car_row_sweep.h", os.path.join(DEV, "car_row_sweep.h"), "static_assert(true ||")):
            cur = open(os.path.join(ge.CSRC, name)).read()
            old = cur
            for was, becomes in rep:
                old = old.replace(was, becomes)
            assert old != cur and old.count(need) == 1, f"{name} no longer has the lines commit 0d74f26 changed"
            open(out_path, "w").write(old)
        # beside it: car_api.hip (errors, the LDS reservation), car_pack.hip (the kernels car_linear_x3_pack launches) and car_round2.hip (size
        # queries car_pack.hip calls) — a library of its own with no symbol left undefined
        for tag, flags in (("", []), ("_bounds", ["-DCAR_BOUNDS"])):
            so = os.path.join(DEV, f"liboldlin16{tag}.so")
            subprocess.check_call([ge._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", *flags, "-I", os.path.join(ROOT, "include"),
                                   "-I", ge.CSRC, srcf, *(os.path.join(ge.CSRC, u) for u in ("car_api.hip", "car_pack.hip", "car_round2.hip")), "-Wl,-z,defs", "-o", so])
            out.append(so)
    return out


if __name__ == "__main__":
    print("\n".join(build("--reintroduce-0d74f26" in sys.argv)))
