"""CPU: the host mirror's warping-function parser (rasr_amd/host/MfccNode.hh): the declarations of RASR's VTLN recipes are accepted,
everything else of the analytic-function grammar is refused with a named message.  Nothing runs on a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "rasr_amd/host/MfccNode.hh"
#include <cstdio>
int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        int w = -1; bool v = false; double f = -1, l = -1; std::string e;
        const bool ok = AmxHost::MfccNode::parseWarpingFunction(argv[i], &w, &v, &f, &l, &e);
        printf("%d %d %d %.17g %.17g %s\n", ok, w, v, f, l, e.c_str());
    }
}
'''
ACCEPTED = {
    "mel": (0, 0, 1.0, 0.0),
    "bark": (1, 0, 1.0, 0.0),
    "nest(linear-2($(warping-factor), 0.875), mel)": (0, 1, 0.0, 0.875),
    "nest(linear-2(1.06, 0.875), bark)": (1, 1, 1.06, 0.875),
    " nest( linear-2( 0.9 ,0.5 ) , mel ) ": (0, 1, 0.9, 0.5),
}
REFUSED = {
    "mel(discretize-argument)": "not supported",
    "nest(linear-3(1.0, 0.5, 0.9), mel)": "not supported",
    "nest(mel, linear-2(1.0, 0.875))": "not supported",
    "nest(linear-2(0, 0.875), mel)": "number > 0",
    "nest(linear-2(-1.1, 0.875), mel)": "number > 0",
    "nest(linear-2(1.1, 1.0), mel)": "interval (0, 1)",
    "nest(linear-2(1.1, 0.875), gammatone)": "not supported",
    "bilinear(0.3)": "not supported",
    "": "not supported",
}


@pytest.fixture(scope="module")
def parser(tmp_path_factory):
    d = tmp_path_factory.mktemp("node")
    src, exe = d / "parse.cc", d / "parse"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, str(src), "-o", str(exe), "-L", os.path.join(ROOT, "rasr_amd"),
                           "-lrasr_amd", "-Wl,-rpath," + os.path.join(ROOT, "rasr_amd")])

    def run(decls):
        out = subprocess.run([str(exe)] + decls, check=True, capture_output=True, text=True).stdout.splitlines()
        return [o.split(" ", 5) for o in out]
    return run


def test_accepted_declarations(parser):
    for d, (w, v, f, l), r in zip(ACCEPTED, ACCEPTED.values(), parser(list(ACCEPTED))):
        assert r[0] == "1", (d, r)
        assert (int(r[1]), int(r[2]), float(r[3]), float(r[4])) == (w, v, f, l), d


def test_refused_declarations_name_the_reason(parser):
    for (d, why), r in zip(REFUSED.items(), parser(list(REFUSED))):
        assert r[0] == "0", d
        assert why in r[5] and "warping-function" in r[5], (d, r[5])
