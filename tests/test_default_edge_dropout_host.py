"""CPU: the algebra of coefficient dropout on the default branch, pinned to the REFERENCE's own operator (oracle O1), not to this
project.  code/Ob_propagation.py:195-196 drops the post-softmax coefficients gamma [E,1]; the value a coefficient multiplies is the
target's own relu(lin_value(x_i)), so under a keep mask the operator's output is

    out[i] = relu(lin_value(x))[i] * s[i],     s[i] = sum over edges e into i of keep[e] / (1 - p) * softmax_i(w)[e]

(0 for a node without in-edges) -- the per-(sample, layer, sensor) scalar the device path multiplies by (include/raindrop_hip.h
"coefficient dropout on the default branch").  The reference's F.dropout is replaced, inside the test, by a function that applies
a GIVEN mask; everything else is the reference's code.  Shape: F = 6 nodes, K = 20 channels, a sparse structure in which node 0 has
no in-edge and node 1 exactly one.  Tolerance: the agreement DESIGN (c) records between O1 and the restatement (1.2e-7 / 2.6e-6)
with a 4x margin -- the coefficient sums against float64 within 4 x 1.2e-7, the outputs within 4 x 2.6e-6 of their max-norm."""
import numpy as np
import pytest
import torch

from oracle import ref_loader

P = 0.3
N, K = 6, 20
# (source, target): node 0 has no in-edge, node 1 exactly one, node 4 a duplicate-free fan-in of four
EDGES = [(0, 1), (0, 2), (1, 2), (3, 2), (2, 3), (5, 3), (0, 4), (1, 4), (2, 4), (4, 4), (5, 5), (3, 5)]


class _FunctionalWithMask:
    """torch.nn.functional for the reference module, with `dropout` applying a given keep mask (everything else passes through)."""

    def __init__(self, keep):
        self.keep, self.calls = keep, 0

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def dropout(self, x, p=0.5, training=True, inplace=False):
        assert training and abs(p - P) < 1e-12 and tuple(x.shape) == (len(EDGES), 1)
        self.calls += 1
        return x * self.keep.view(-1, 1).to(x.dtype) / (1.0 - p)


def _case():
    rng = np.random.default_rng(11)
    ei = torch.tensor(EDGES, dtype=torch.int64).t().contiguous()
    ew = torch.from_numpy(rng.uniform(0.5, 1.5, len(EDGES)).astype(np.float32))
    x = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32))
    return ei, ew, x


@pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present")
@pytest.mark.parametrize("keep_bits", [0b101101110101, 0b111111111111, 0b000000000010, 0b010010101010])
def test_reference_operator_under_a_keep_mask_is_the_per_target_scale(monkeypatch, keep_bits):
    ref = ref_loader.load()
    torch.manual_seed(3)
    op = ref.run(ref.Ob_propagation.Observation_progation, in_channels=K, out_channels=K, heads=1, n_nodes=N, ob_dim=4)
    op.dropout = P                                     # what upstream users set: the constructor call of the model has no keyword
    op.train()
    ei, ew, x = _case()
    keep = torch.tensor([(keep_bits >> e) & 1 for e in range(len(EDGES))], dtype=torch.float32)
    fake = _FunctionalWithMask(keep)
    monkeypatch.setattr(ref.Ob_propagation, "F", fake)
    with torch.no_grad():
        out, (ei_ret, alpha) = ref.run(op.forward, x, None, ei, edge_weights=ew, use_beta=False, return_attention_weights=True)
        v = torch.relu(op.lin_value(x))
    assert fake.calls == 1
    # the formula, in float64 from the raw weights
    w, tgt = ew.double().numpy(), ei[1].numpy()
    s = np.zeros(N)
    for i in range(N):
        into = np.nonzero(tgt == i)[0]
        if len(into):
            g = np.exp(w[into] - w[into].max())
            g = g / (g.sum() + 1e-16)
            s[i] = float((keep.numpy()[into].astype(np.float64) / (1.0 - P) * g).sum())
    assert s[0] == 0.0                                                     # no in-edge: nothing arrives
    one = int(np.nonzero(tgt == 1)[0][0])
    assert abs(s[1] - float(keep[one]) / (1.0 - P)) <= 4 * 1.2e-7          # one in-edge: softmax 1, kept or dropped whole
    want = v.double().numpy() * s[:, None]
    got = out.double().numpy()
    assert got.shape == (N, K)
    assert np.abs(got - want).max() <= 4 * 2.6e-6 * max(np.abs(want).max(), 1.0), float(np.abs(got - want).max())
    # the scale itself, read back from the output where the value is not 0
    nz = np.abs(v.numpy()) > 1e-3
    ratio = np.where(nz, got / np.where(nz, v.double().numpy(), 1.0), 0.0)
    for i in range(N):
        if nz[i].any():
            assert np.abs(ratio[i][nz[i]] - s[i]).max() <= 4 * 2.6e-6 * max(s[i], 1.0), i
    # returned values: the list as given and the PRE-dropout (pre-softmax) weights
    assert torch.equal(ei_ret, ei) and torch.equal(alpha.view(-1), ew)


def test_helper_reads_the_two_attributes_in_training_mode_only():
    """raindrop_amd.models_rd.coef_dropout_of: (p1, p2) in training mode, (0, 0) in evaluation mode; out-of-range values raise."""
    from raindrop_amd import _lib
    from raindrop_amd.models_rd import Raindrop_v2, coef_dropout_of
    m = Raindrop_v2(d_inp=5, d_model=20, nhead=2, nhid=16, nlayers=1, dropout=0.0, max_len=7, d_static=3, n_classes=2,
                    global_structure=torch.ones(5, 5))
    assert coef_dropout_of(m.train()) == (0.0, 0.0)
    m.ob_propagation.dropout, m.ob_propagation_layer2.dropout = 0.3, 0.5
    assert coef_dropout_of(m.train()) == (0.3, 0.5)
    assert coef_dropout_of(m.eval()) == (0.0, 0.0)
    m.ob_propagation_layer2.dropout = 1.0
    with pytest.raises(_lib.RaindropHipError):
        coef_dropout_of(m.train())
