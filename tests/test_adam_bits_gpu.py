"""GPU: the bits of the Adam update, pinned.  Which product of `b1 * m + (1 - b1) * gr` the compiler fuses into an FMA is its
choice, and it follows details of the source as small as the order of the loads (csrc/rd_optim.hip adam_thread).  The digests in
tests/golden/adam_update_bits.json were taken from the library as it was BEFORE the eight forms of the update shared one body; every
form must still give them -- a change of the update that means to change the bits regenerates the file and says so."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_update_bits.json")
# form -> (FlatAdam method, keywords): the eight entry points rd_adam_step [_clip] [_ema] [_dev]
FORMS = {"plain": ("step", {}), "dev": ("step_captured", {}),
         "clip": ("step", dict(max_grad_norm=1.0)), "clip_dev": ("step_captured", dict(max_grad_norm=1.0)),
         "ema": ("step", dict(ema_decay=0.9)), "ema_dev": ("step_captured", dict(ema_decay=0.9)),
         "clip_ema": ("step", dict(max_grad_norm=1.0, ema_decay=0.9)),
         "clip_ema_dev": ("step_captured", dict(max_grad_norm=1.0, ema_decay=0.9))}
N, STEPS = 1027, 3                                                  # float4 slots in five workgroups and a three-element scalar tail


def update_digests():
    """{form: sha256 over the bytes of p, exp_avg, exp_avg_sq (and ema) after STEPS steps on seeded data}"""
    from raindrop_amd.optim import FlatAdam
    out = {}
    for form, (method, kw) in FORMS.items():
        g_ = torch.Generator(device="cpu").manual_seed(11)
        p = torch.nn.Parameter(torch.randn(N, generator=g_).to("cuda"))
        p.grad = torch.zeros(N, device="cuda")
        opt = FlatAdam(p, lr=1e-2, weight_decay=0.01, **kw)
        if method == "step_captured":
            opt.sync_step_cell()
        for _ in range(STEPS):
            p.grad.copy_(torch.randn(N, generator=g_).to("cuda"))
            if method == "step":
                opt.step()
            else:
                opt.step_captured(); opt.note_replay()
        h = hashlib.sha256()
        for t in (p.detach(), opt.exp_avg, opt.exp_avg_sq) + ((opt.ema,) if opt.ema is not None else ()):
            h.update(t.cpu().numpy().tobytes())
        out[form] = h.hexdigest()
    return out


def test_every_form_gives_the_recorded_bits():
    want = json.load(open(GOLDEN))
    got = update_digests()
    assert sorted(got) == sorted(want)
    assert [f for f in got if got[f] != want[f]] == []
