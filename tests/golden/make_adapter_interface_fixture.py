"""Generates tests/golden/adapter_interface.json: the interfaces of the reference that adapter/ implements, as data --
the pure virtuals (name, parameter types) of TransImpl (src/atlas/trans/detail/TransImpl.h), VorDivToUVImpl
(src/atlas/trans/VorDivToUV.h) and LegendreCacheCreatorImpl (src/atlas/trans/LegendreCacheCreator.h), and the setup
overloads and execute templates of parallel::HaloExchange (src/atlas/parallel/HaloExchange.h).  Extracted with the same
parsing as tests/test_adapter_source.py, which compares the adapter against this file.

    python tests/golden/make_adapter_interface_fixture.py PATH_OF_AN_ATLAS_0.44.1_SOURCE_CHECKOUT"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from test_adapter_source import HALO_EXECUTE, PURE_VIRTUAL, _methods, _norm_params  # noqa: E402

OUT = os.path.join(HERE, "adapter_interface.json")


def pure_virtuals(text, begin, end=None):
    text = text[text.index(begin):text.index(end) if end else None]
    return sorted([name, list(params)] for name, params in _methods(text, PURE_VIRTUAL))


def main(src):
    def read(rel):
        with open(os.path.join(src, "src", "atlas", rel)) as f:
            return f.read()
    halo = read("parallel/HaloExchange.h")
    halo = halo[halo.index("class HaloExchange"):halo.index("private:  // methods")]
    out = {
        "TransImpl": pure_virtuals(read("trans/detail/TransImpl.h"), "class TransImpl"),
        "VorDivToUVImpl": pure_virtuals(read("trans/VorDivToUV.h"), "class VorDivToUVImpl", "class VorDivToUVFactory"),
        "LegendreCacheCreatorImpl": pure_virtuals(read("trans/LegendreCacheCreator.h"), "class LegendreCacheCreatorImpl",
                                                  "class LegendreCacheCreator :"),
        "HaloExchange": {
            "setup": sorted(list(_norm_params(m.group(1))) for m in re.finditer(r"void\s+setup\(([^)]*)\)", halo)),
            "execute_templates": [name for name in ("execute", "execute_adjoint") if re.search(HALO_EXECUTE % name, halo)],
        },
    }
    with open(OUT, "w") as f:   # one signature per line
        f.write("{\n" + ",\n".join(
            f" {json.dumps(k)}: " + ("[\n" + ",\n".join("  " + json.dumps(e) for e in v) + "\n ]" if isinstance(v, list) else
                                     "{\n" + ",\n".join(f"  {json.dumps(kk)}: {json.dumps(vv)}" for kk, vv in v.items()) + "\n }")
            for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
