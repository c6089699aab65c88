#!/usr/bin/env python
"""Record how the REFERENCE behaves where a test states a claim about it, so that the test needs no reference sources:

    tests/golden/reference_probes.json    {probe name: the probe's stdout}

frame_variant_code: the reference generator called with the (B, D, T) clip code that VOICE2POSE.GENERATOR.CLIP_CODE.FRAME_VARIANT produces
(tests/test_host_logic.py::test_frame_variant_codes_are_rejected_like_the_reference_rejects_them).
Run where the reference sources are:  python tests/golden/make_reference_probes.py <reference checkout>
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PROBES = {
    "frame_variant_code": (
        "import torch\nfrom types import SimpleNamespace as NS\nfrom core.networks import get_model\n"
        "cfg = NS(VOICE2POSE=NS(GENERATOR=NS(LEAKY_RELU=True, NORM='IN', CLIP_CODE=NS(DIMENSION=32))), DATASET=NS(NUM_LANDMARKS=121))\n"
        "G = get_model('SequenceGeneratorCNN')(cfg)\n"
        "try:\n    G(torch.randn(1, 80, 427), 64, torch.randn(1, 32, 64))\n    print('ACCEPTED')\n"
        "except RuntimeError as e:\n    print('RAISES', e)\n"),
}


def main(ref):
    out = {}
    for name, code in PROBES.items():
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=HERE,
                           env=dict(os.environ, PYTHONPATH=os.path.abspath(ref), PYTHONDONTWRITEBYTECODE="1"))
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = r.stdout.strip()
    path = os.path.join(HERE, "reference_probes.json")
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    print("wrote", path, out)


if __name__ == "__main__":
    main(sys.argv[1])
