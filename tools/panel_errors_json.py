#!/usr/bin/env python3
"""profiles/panel_float64_errors.json from the output of `pytest tests/test_panel_float64_gpu.py -s`.

    python -m pytest tests/test_panel_float64_gpu.py -q -s -m gpu > panel64.log
    python tools/panel_errors_json.py panel64.log profiles/panel_float64_errors.json

Every `panel64 <kind> <case> <form> <mode>: <tensor> <error>, ...` line becomes one record with each tensor's error and its ratio
to the bound the test applies (tests/sensor_stage_ref.py bound_of for the stage, tests/dropout_ref.py enc_bound for the encoder
layer); the worst ratio per form and the largest of all are stated on top.  The `panel16` lines of the one-product bf16 mode are
kept as printed, next to the CPU-computed pairwise bound (tests/panel_ref.py pair_sum).  No bound comes from these figures."""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import dropout_ref as DR            # noqa: E402
from tests import panel_ref as PR              # noqa: E402
from tests import sensor_stage_ref as SR       # noqa: E402

LINE16 = re.compile(r"panel16 (stage|pair) (\S+) (\S+) bf16: (.*)$")
LINE = re.compile(r"panel64 (stage|guard|encoder) (\S+) (small|wide|pc) (bf16x3): (.*)$")


def main(log, out):
    stage_bound, enc_bound = SR.bound_of("bf16x3"), DR.enc_bound("bf16x3")
    runs, worst, runs16 = [], {}, []
    for line in open(log):
        m16 = LINE16.search(line.strip())
        if m16:                                        # one-product mode: the line as printed (errors, ratio to the element-wise bound)
            runs16.append({"kind": m16.group(1), "case": m16.group(2), "forms": m16.group(3), "mode": "bf16", "figures": m16.group(4)})
            continue
        m = LINE.search(line.strip())                  # behind the progress dots of -q
        if not m:
            continue
        kind, case, form, mode, rest = m.groups()
        tensors = {}
        for item in rest.split(", "):
            name, err = item.rsplit(" ", 1)
            metric, bound = (enc_bound if kind == "encoder" else stage_bound)(name)
            if name.endswith("/max"):                  # the encoder gradients' second assertion: max-norm at the gate-free ties' 2e-4
                metric, bound = "rel", SR.GRAD_REL
            e = float(err)
            tensors[name] = {"error": e, "metric": metric, "bound": bound, "ratio": round(e / bound, 4)}
            w = worst.setdefault(form, {"ratio": 0.0})
            if e / bound > w["ratio"]:
                worst[form] = {"ratio": round(e / bound, 4), "tensor": name, "case": case, "kind": kind}
        runs.append({"kind": kind, "case": case, "form": form, "mode": mode, "tensors": tensors})
    assert runs, "no panel64 line in " + log
    doc = {
        "device": "AMD Instinct MI355X (gfx950)",
        "source": "tests/test_panel_float64_gpu.py -s",
        "metric": {"z": "max absolute error over z_scale(reference) (sensor_stage_ref.z_scale)", "pe": "max absolute error",
                   "stage gradients": "max error over the float64 tensor's max-norm",
                   "encoder y": "max absolute error", "encoder gradients": "relative L2 error"},
        "bounds": {"stage": {"z": SR.Z_ABS["bf16x3"], "pe": SR.PE_ABS, "gradients": SR.GRAD_REL},
                   "encoder": {"y": enc_bound("y")[1], "gradients": enc_bound("x")[1]}},
        "one_product_bf16_mode": {
            "reference": "float64 sums of bf16-rounded operands (tests/panel_ref.py evaluate16), biases gap-placed in that arithmetic",
            "z bound": "element-wise: 2e-5 x 6 x z_scale + one flipped bf16 rounding of Y1 in the row (s2 max_k ulp(Y1[r,k]) |W2[n,k]|)",
            "gradient bound": "relative L2 2e-2 and max-norm 0.25 (test_sensor_stage_vs_oracle, bf16 modes)",
            "pairwise_bound_cpu": {"value": PR.pair_sum()[0], "per_case_order_difference": PR.pair_sum()[1],
                                   "how": "4 x max |chunk order - even / odd chunk order| of the fp32 sums of the reference's bf16-rounded "
                                          "products, both forward products, computed on the CPU; plus the one-flip term per element"},
            "runs": runs16},
        "largest_ratio": max(w["ratio"] for w in worst.values()),
        "worst": worst,
        "runs": runs,
    }
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("%d runs, largest ratio %.3f" % (len(runs), doc["largest_ratio"]))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
