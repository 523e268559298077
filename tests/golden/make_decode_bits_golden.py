"""Records tests/golden/decode_bits_v1.json: what the fused decode kernels write, bit for bit, on the cases of
tests/test_decode_bits_gpu.py (sha256 per output array, tokens in clear) with the sha256 of every input.  Needs the GPU.

The committed fixture was taken at the commit it names, the last one whose decode.hip stated the LM-head body twice and every
weight-stream loop once per weight format.  It is not meant to be regenerated from the current tree: only a change that MEANS to
move the bits (a new summation order, another k-to-lane map) records it again, from the tree it leaves, and says so.

  python tests/golden/make_decode_bits_golden.py <commit> [<output file>]
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import torch

from lap_amd import hip
from tests import decode_reference as C
from tests import test_decode_bits_gpu as T


def main():
    results = {}
    for form in C.LM_FORMS:
        results.update(T.lm_results(hip, form))
    for kind in T.PROJECTIONS:
        for wt in T.WEIGHTS:
            results.update(T.projection_results(hip, kind, wt))
    fixture = {"commit": sys.argv[1], "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "inputs": T.input_hashes(),
               "results": results}
    out = pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else T.FIXTURE
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(fixture, indent=1) + "\n")
    print(len(results), "cases ->", out)


if __name__ == "__main__":
    main()
