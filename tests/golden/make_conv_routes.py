"""Record tests/golden/conv_routes.json: the answers of the convolution size queries and the route every operator takes
(tests/route_cases.py), from THIS checkout's own libraries.  Run it at the commit whose behaviour is the contract, never to make a
failing tests/test_conv_routes_*.py pass.

    python tests/golden/make_conv_routes.py          # host emulator library: "queries" and "routes_emu"
    python tests/golden/make_conv_routes.py --gpu    # gfx950 measurement library on a GPU: "routes_gpu" (the other sections are kept)
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS, os.path.join(TESTS, "emu")]
os.environ.setdefault("NEMAR_AB_LIBRARY", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    a = ap.parse_args()
    import route_cases as RC
    from nemar_amd import _lib
    table = RC.load_table() if os.path.exists(RC.TABLE) else {}
    if a.gpu:
        from backends import HipBackend
        table["routes_gpu"] = RC.route_table(HipBackend(_lib.load()), RC.GPU_SHAPES, lift=False)
    else:
        import build_emu
        from backends import EmuBackend
        lib = _lib.load(build_emu.build())
        table["queries"] = RC.query_table(lib)
        table["routes_emu"] = RC.route_table(EmuBackend(lib), RC.SMALL_SHAPES, lift=True)
    with open(RC.TABLE, "w") as f:
        f.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (sec, ",\n".join('  "%s": %s' % (k, json.dumps(v)) for k, v in table[sec].items()))
                                   for sec in sorted(table)) + "\n}\n")
    print("wrote %s: %s" % (RC.TABLE, ", ".join("%s (%d)" % (s, len(table[s])) for s in sorted(table))))


if __name__ == "__main__":
    main()
