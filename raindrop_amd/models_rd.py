"""`models_rd` surface of the reference (code/models_rd.py) on MI355X-native kernels.

Drop-in boundary: `code/Raindrop.py:19` does `from models_rd import *`,
constructs `Raindrop_v2(...)` positionally (`:245-251`), calls `.cuda()`, `.parameters()`,
`.train()/.eval()`, `model.forward(P, Pstatic, Ptime, lengths)` (`:319`) and
`state_dict()/load_state_dict()` (`:374,381`).  The classes below keep those signatures, the
parameter names/shapes (dead parameters included) and the return tuple; the
arithmetic is issued as HIP kernels through `raindrop_amd.ops` -- there is no eager fallback.

Differences from the reference, all deliberate and documented in DESIGN.md:
  * `R_u` is a registered Parameter (the reference loses it on GPU through
    `Parameter(...).cuda()`, code/models_rd.py:241; on CPU it IS registered);
  * no host round trips in forward (PE, padding mask and the edge list are built on device);
  * the caller's `global_structure` is not mutated (the reference writes its diagonal in place
    on CPU, code/models_rd.py:307-308);
  * `distance` is the exact constant 0 the reference computes on this path; on the paper's branch
    (`use_beta=True, compute_distance=True`) it is the reference's differentiable regulariser.
"""
import ctypes

import torch
import torch.nn as nn
from torch.nn.parameter import Parameter

from . import _lib, graph_module, ops
from .Ob_propagation import Observation_progation, glorot
from .transformer_conv import TransformerConv

__all__ = ["PositionalEncodingTF", "Raindrop", "Raindrop_v2", "Observation_progation", "TransformerConv"]


class PositionalEncodingTF(nn.Module):
    """code/models_rd.py:20-43: sinusoidal encoding of continuous timestamps, timescales
    `max_len ** linspace(0, 1, d_model/2)`.  Computed on device (the reference goes through the
    host); returns [T, B, d_model]."""

    def __init__(self, d_model, max_len=500, MAX=10000):
        super().__init__()
        self.max_len = max_len
        self.d_model = d_model
        self.MAX = MAX
        self._num_timescales = d_model // 2
        self._ts = {}

    def timescales(self, device):
        key = str(device)
        if key not in self._ts:
            self._ts[key] = ops.timescales(self.max_len, self.d_model).to(device)
        return self._ts[key]

    def getPE(self, P_time):
        T, B = P_time.shape
        shp = _lib.shape(B, T, 1, 1, d_pe=self.d_model)
        z = torch.empty((T, B, 1 + self.d_model), dtype=torch.float32, device=P_time.device)
        mask = torch.empty((B, T), dtype=torch.bool, device=P_time.device)
        lengths = torch.zeros((B,), dtype=torch.int64, device=P_time.device)
        times = P_time.contiguous().float()          # keep alive until the launch is enqueued
        ts = self.timescales(P_time.device)
        _lib.call("rd_pe_mask", ctypes.byref(shp), ops._ptr(times), ops._ptr(lengths), ops._ptr(ts),
                  ops._ptr(z), ops._ptr(mask), ops._stream())
        return z[:, :, 1:]

    def forward(self, P_time):
        return self.getPE(P_time)


class Raindrop(nn.Module):
    """code/models_rd.py:46-191 -- the legacy model `from models_rd import *` also exports (never constructed by
    code/Raindrop.py).  A `Linear(d_inp, 36)` input encoder scaled by sqrt(d_model), a `TransformerConv` applied per sample to the
    [T, 36] step matrix (its NODES are the time steps, the sensor graph's edges connect the first 36 of them -- as upstream), a
    36-wide positional encoding, the temporal encoder, the masked mean and the static head.  Same constructor signature,
    registration order and state_dict surface; the per-sample Python loop of :155-165 is one batched operator call.
    Upstream hard-codes 36 sensors and 215 steps inside forward (:150,:155); the sizes are read from the inputs here, and the
    width relations upstream relies on (d_model a multiple of d_inp = 36) are checked at construction."""

    def __init__(self, d_inp=36, d_model=64, nhead=4, nhid=128, nlayers=2, dropout=0.3, max_len=215, d_static=9,
                 MAX=100, perc=0.5, aggreg='mean', n_classes=2, global_structure=None):
        super().__init__()
        from torch.nn import TransformerEncoder, TransformerEncoderLayer
        self.model_type = 'Transformer'
        self.global_structure = global_structure
        d_pe = 36
        d_enc = 36
        self.d_pe = d_pe
        self.pos_encoder = PositionalEncodingTF(d_pe, max_len, MAX)
        encoder_layers = TransformerEncoderLayer(d_model + 36, nhead, nhid, dropout)
        self.transformer_encoder = TransformerEncoder(encoder_layers, nlayers, enable_nested_tensor=False)
        self.gcs = nn.ModuleList()
        self.dim = int(d_model / d_inp)
        self.transconv = TransformerConv(in_channels=36, out_channels=36 * self.dim, heads=1)
        d_final = 36 * (self.dim + 1) + d_model
        self.mlp_static = nn.Sequential(nn.Linear(d_final, d_final), nn.ReLU(), nn.Linear(d_final, n_classes))
        self.d_inp = d_inp
        self.d_model = d_model
        self.encoder = nn.Linear(d_inp, d_enc)
        self.emb = nn.Linear(d_static, d_model)
        self.MLP_replace_transformer = nn.Linear(72, 36)                                   # dead (:98)
        self.mlp = nn.Sequential(nn.Linear(d_model, d_model), nn.ReLU(), nn.Linear(d_model, n_classes))   # dead (:100-104)
        self.aggreg = aggreg
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(dropout)
        self.nhead, self.nhid, self.nlayers, self.max_len = nhead, nhid, nlayers, max_len
        self.n_classes, self.d_static = n_classes, d_static
        self._graph_cache = None
        self._drop_calls = 0
        # upstream hard-wires 36 everywhere (code/models_rd.py:75-84: TransformerConv(in_channels=36), Linear(d_inp, 36), a 36-wide
        # encoding) while forward slices src[:, :, :d_inp]: only d_inp = 36 is a consistent model
        if d_inp != 36:
            raise _lib.RaindropHipError("Raindrop (legacy): d_inp = %d is unsupported (RD_EUNSUPPORTED) -- upstream hard-wires 36 "
                                        "sensors (code/models_rd.py:75-84: TransformerConv(in_channels=36), Linear(d_inp, 36)); "
                                        "use Raindrop_v2 for other sensor counts" % d_inp)
        if d_inp * self.dim != d_model:
            raise _lib.RaindropHipError("Raindrop (legacy): d_model (%d) must be a multiple of d_inp (%d) -- upstream concatenates a "
                                        "[.., 36*int(d_model/d_inp)] graph output with a 36-wide encoding for an encoder of "
                                        "width d_model + 36 (code/models_rd.py:75,84,168)" % (d_model, d_inp))
        self.init_weights()

    def init_weights(self):
        """code/models_rd.py:110-113."""
        initrange = 1e-10
        self.encoder.weight.data.uniform_(-initrange, initrange)
        self.emb.weight.data.uniform_(-initrange, initrange)

    def _graph(self, device):
        gs = self.global_structure
        key = (str(device), gs.data_ptr(), gs._version)
        if self._graph_cache is None or self._graph_cache[0] != key:
            adj, ei, ew = ops.graph_build(gs.to(device=device, dtype=torch.float32))        # :147-151 (diagonal set, nonzero order)
            self._graph_cache = (key, dict(adj=adj, edge_index=ei, edge_weights=ew))
        return self._graph_cache[1]

    def forward(self, src, static, times, lengths):
        """src [T,B,2*d_inp], static [B,d_static], times [T,B], lengths [B] -> (logits, distance, None) -- code/models_rd.py:115-191."""
        if not src.is_cuda:
            raise _lib.RaindropHipError("Raindrop runs on a ROCm device only; move inputs with .cuda()")
        import math
        dev = src.device
        T, B = src.shape[0], src.shape[1]
        p_drop = float(self.dropout.p) if self.training else 0.0
        self._drop_calls += 1
        seed = (torch.initial_seed() * 1000003 + self._drop_calls + ops.rank_seed_offset()) & 0x7FFFFFFFFFFFFFFF
        lengths = lengths.to(device=dev, dtype=torch.int64)
        vals = src[:, :, :self.d_inp].float().contiguous().view(T * B, self.d_inp)          # :126 (layout only)
        x = ops.linear(vals, self.encoder.weight, self.encoder.bias)                         # :129
        x = ops.scale_dropout(x, math.sqrt(self.d_model), p_drop, seed, site=2)              # :129,:134
        n_feat = self.encoder.out_features
        x = x.view(T, B, n_feat).permute(1, 0, 2).contiguous()                               # [B, T nodes, 36]: layout only
        g = self._graph(dev)
        C = 36 * self.dim
        shp = _lib.shape(B, T, 36, self.dim, d_pe=self.d_pe, nhead=self.nhead, nhid=self.nhid, d_static=self.d_static,
                         n_classes=self.n_classes, max_len=self.max_len)
        # PE columns + padding mask straight into the encoder's input buffer (:131,:143-144,:168)
        z = torch.empty((T, B, C + self.d_pe), dtype=torch.float32, device=dev)
        mask = torch.empty((B, T), dtype=torch.bool, device=dev)
        tt = times.float().contiguous()
        ts = self.pos_encoder.timescales(dev)
        _lib.call("rd_pe_mask", ctypes.byref(shp), ops._ptr(tt), ops._ptr(lengths), ops._ptr(ts), ops._ptr(z), ops._ptr(mask),
                  ops._stream())
        out = self.transconv(x, g["edge_index"], edge_weights=g["edge_weights"], edge_attr=None, return_attention_weights=True)[0]
        # [B,T,C] -> columns [0, C) of z[T,B,:]: the per-sample assignment of :162 as one layout kernel (F = 1 "sensor" of C channels
        # per step would transpose nothing: rows_to_tokens with T steps of one C-wide cell)
        shp_l = _lib.shape(B, T, 1, C, d_pe=self.d_pe)
        z = ops.rows_to_tokens(out.reshape(B, 1, T * C), None, z, shp_l)
        distance = torch.zeros((), dtype=torch.float32, device=dev)    # every sample returns the same coefficients: cdist == 0 (:166-167)
        r_out = z
        for i, layer in enumerate(self.transformer_encoder.layers):
            named = dict(layer.named_parameters())
            r_out = ops.encoder_layer(r_out, mask, shp, i, p_drop, seed, [named[n] for n in ops.ENC_PARAM_NAMES])
        emb = ops.linear(static.float(), self.emb.weight, self.emb.bias)                     # :135
        agg = ops.masked_mean(r_out, mask, lengths, shp)                                     # :178-183
        output = torch.cat([agg, emb], dim=1)                                                # :187
        hid = ops.linear(output, self.mlp_static[0].weight, self.mlp_static[0].bias, act=1)
        output = ops.linear(hid, self.mlp_static[2].weight, self.mlp_static[2].bias)
        return output, distance, None


def edge_dropout_of(model):
    """Layer 1's coefficient-dropout probability of a use_beta model: `ob_propagation.dropout` in training mode, 0 in evaluation
    mode.  Layer 2's (`ob_propagation_layer2.dropout > 0`, training mode) is refused: its dropped coefficients no longer sum to 1
    per target, so the edge scores get a gradient through them that no backward of this project forms."""
    if not model.training:
        return 0.0
    if float(model.ob_propagation_layer2.dropout) > 0.0:
        raise _lib.RaindropHipError("RD_EUNSUPPORTED: ob_propagation_layer2.dropout > 0 with use_beta=True in training mode is not "
                                    "built (the gradient of layer 2's dropped coefficient sum w.r.t. the edge scores)")
    return float(model.ob_propagation.dropout)


def coef_dropout_of(model):
    """(p1, p2), the coefficient-dropout probabilities of the two operators on the DEFAULT branch (`use_beta=False`):
    `ob_propagation.dropout` / `ob_propagation_layer2.dropout` in training mode (code/Ob_propagation.py:195-196; upstream users set
    the attributes, the constructor has no keyword for them), (0, 0) in evaluation mode.  The edge weights of this branch come from
    `global_structure`, which is no parameter: dropping coefficients adds no gradient term, and both layers are supported."""
    if not model.training:
        return 0.0, 0.0
    p1, p2 = float(model.ob_propagation.dropout), float(model.ob_propagation_layer2.dropout)
    if not (0.0 <= p1 < 1.0 and 0.0 <= p2 < 1.0):
        raise _lib.RaindropHipError("ob_propagation.dropout / ob_propagation_layer2.dropout must be in [0, 1), got %r" % ((p1, p2),))
    return p1, p2


class Raindrop_v2(nn.Module):
    """code/models_rd.py:194-387.  Transformer-over-time on top of per-sample sensor-graph message
    passing; see the module docstring for the boundary contract."""

    def __init__(self, d_inp=36, d_model=64, nhead=4, nhid=128, nlayers=2, dropout=0.3, max_len=215,
                 d_static=9, MAX=100, perc=0.5, aggreg='mean', n_classes=2, global_structure=None,
                 sensor_wise_mask=False, static=True, freeze_R_u=False, use_beta=False, compute_distance=False):
        """Positional signature of code/models_rd.py:208-209.  `freeze_R_u` (keyword, not in the reference): the
        upstream GPU run builds `R_u = Parameter(...).cuda()`, a NON-leaf tensor -- it never reaches the optimizer or
        the state_dict and keeps its initial value.  Here R_u is a registered, trained Parameter
        (the evident intent); `freeze_R_u=True` restores the upstream dynamics (requires_grad=False, still saved).

        `use_beta` / `compute_distance` (keywords, defaults = the reference's literals): the reference hard-wires
        `use_beta = False` inside forward (code/models_rd.py:317) and always evaluates `distance`, which is exactly 0 on
        that path.  `use_beta=True` runs the paper's branch -- layer 1 through
        `Observation_progation.message`'s use_beta arm (time-dependent edge scores from the positional encoding, half of
        the edges pruned PER SAMPLE), layer 2 on each sample's surviving edges -- and `compute_distance=True` evaluates
        code/models_rd.py:345-346 on the returned edge scores instead of returning the constant.  That `distance` is
        differentiable, as the reference's is: `(ce + lam * distance).backward()` trains the paper's objective (the gradient
        reaches R_u, increase_dim and map_weights of layer 1 through the edge scores); a loss without it is unchanged."""
        super().__init__()
        from torch.nn import TransformerEncoder, TransformerEncoderLayer
        self.model_type = 'Transformer'
        self.global_structure = global_structure
        self.sensor_wise_mask = sensor_wise_mask
        self.use_beta = bool(use_beta)
        self.compute_distance = bool(compute_distance)
        if sensor_wise_mask:
            raise _lib.RaindropHipError(
                "RD_EUNSUPPORTED: sensor_wise_mask=True is broken in the reference itself (shape "
                "mismatch in mlp_static) and hard-wired off at code/Raindrop.py:103")
        d_pe = 16
        self.d_pe = d_pe
        self.d_inp = d_inp
        self.d_model = d_model
        self.static = static
        self.nhead = nhead
        self.nhid = nhid
        self.nlayers = nlayers
        self.max_len = max_len
        self.n_classes = n_classes
        self.d_static = d_static
        # registration order mirrors code/models_rd.py:223-264
        if self.static:
            self.emb = nn.Linear(d_static, d_inp)
        self.d_ob = int(d_model / d_inp)
        self.encoder = nn.Linear(d_inp * self.d_ob, self.d_inp * self.d_ob)          # dead (:228)
        self.pos_encoder = PositionalEncodingTF(d_pe, max_len, MAX)
        encoder_layers = TransformerEncoderLayer(d_model + 16, nhead, nhid, dropout)
        self.transformer_encoder = TransformerEncoder(encoder_layers, nlayers, enable_nested_tensor=False)
        self.R_u = Parameter(torch.Tensor(1, self.d_inp * self.d_ob))
        self.ob_propagation = Observation_progation(
            in_channels=max_len * self.d_ob, out_channels=max_len * self.d_ob, heads=1,
            n_nodes=d_inp, ob_dim=self.d_ob)
        self.ob_propagation_layer2 = Observation_progation(
            in_channels=max_len * self.d_ob, out_channels=max_len * self.d_ob, heads=1,
            n_nodes=d_inp, ob_dim=self.d_ob)
        d_final = d_model + d_pe + (d_inp if static else 0)
        self.mlp_static = nn.Sequential(nn.Linear(d_final, d_final), nn.ReLU(), nn.Linear(d_final, n_classes))
        self.mlp = nn.Sequential(nn.Linear(d_model, d_model), nn.ReLU(), nn.Linear(d_model, n_classes))  # dead
        self.aggreg = aggreg
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(dropout)
        self._graph_cache = None
        self._drop_calls = 0
        self.init_weights()
        if freeze_R_u:
            self.R_u.requires_grad_(False)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Checkpoints written by the reference on a GPU have no `R_u` entry (non-leaf tensor, see __init__): loading
        them keeps this model's R_u instead of failing `strict=True`."""
        key = prefix + "R_u"
        if key not in state_dict:
            import warnings
            warnings.warn("Raindrop_v2.load_state_dict: the checkpoint has no `R_u` (a reference GPU checkpoint: upstream R_u is a non-leaf "
                          "tensor that is never saved, code/models_rd.py:241).  The model that wrote it used ITS OWN glorot draw of R_u, which "
                          "the file does not contain; this model keeps its current R_u, so its logits will differ from the writer's unless "
                          "R_u is restored separately (same torch seed at construction, or assign model.R_u.data).", stacklevel=3)
            state_dict = dict(state_dict)
            state_dict[key] = self.R_u.detach()
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def __getstate__(self):
        """pickling / copy.deepcopy: the captured step's runners (hipGraphs, raindrop_amd/graph_module.py) stay behind; a copy
        captures its own on its first training call"""
        d = dict(self.__dict__)
        d.pop("_graph_runners", None)
        d.pop("_eval_steps", None)                                 # raindrop_amd.feed.evaluate_captured's cached forwards
        return d

    def init_weights(self):
        """code/models_rd.py:271-276."""
        initrange = 1e-10
        self.encoder.weight.data.uniform_(-initrange, initrange)
        if self.static:
            self.emb.weight.data.uniform_(-initrange, initrange)
        glorot(self.R_u)

    # -- sensor graph (code/models_rd.py:307-311), cached per (device, structure version) ------
    def _graph(self, device):
        gs = self.global_structure
        key = (str(device), gs.data_ptr(), gs._version)
        if self._graph_cache is None or self._graph_cache[0] != key:
            adj, ei, ew = ops.graph_build(gs.to(device=device, dtype=torch.float32))
            gamma, ssum = ops.edge_softmax_dense(adj)
            self._graph_cache = (key, dict(adj=adj, edge_index=ei, edge_weights=ew, gamma=gamma, ssum=ssum))
        return self._graph_cache[1]

    def forward_seed(self, calls):
        """The dropout seed of the forward that is this model's `calls`-th (`_drop_calls` after it): every mask of that forward --
        observation embedding, encoder, the use_beta operators' coefficients -- is a function of it.  A captured step whose
        seed + seed cell equals it draws the same masks."""
        return (torch.initial_seed() * 1000003 + int(calls) + ops.rank_seed_offset()) & 0x7FFFFFFFFFFFFFFF

    def _sensor_stage_beta(self, src, times, lengths, shp, p_drop, seed, g):
        """code/models_rd.py:313-346 with `use_beta = True`, batched over the samples (the reference loops):
        X = dropout(relu(src * R_u)) as [B,F,K]; layer 1 = the use_beta operator with p_t = the sample's positional
        encoding (:324,:329) -> per-sample pruned edge lists and scores; layer 2 = the default branch on THOSE lists
        (:331-336): relu(lin_value(y1_i)) * sum of the per-target softmax over the surviving edges into i (1 where a
        target keeps an edge, 0 where pruning removed them all); then the [F,T*d] -> [T,F*d] layout and the PE columns.
        `distance` = mean pairwise distance of the samples' returned scores (:345-346) when `compute_distance`, differentiable
        through those scores (ops.graph_beta(alpha_grad=True) -> ops.structure_distance).  Layer 2's edge weights stay constants:
        the per-target softmax over them sums to 1 (or is absent), so their true gradient is 0.
        Coefficient dropout (training mode only): `self.ob_propagation.dropout` drops layer 1's post-softmax coefficients (four keep
        decisions per (sample, edge, step): rd_graph_beta_fwd_dropout) under the forward's one `seed`; upstream users set the
        attribute, the constructor has no keyword for it.  `self.ob_propagation_layer2.dropout > 0` is refused in training mode
        (edge_dropout_of): with it layer 2's coefficient sum is no longer 1, its edge weights get a true gradient through
        d ssum / d alpha, and the constant treatment above would silently drop that term."""
        dev = src.device
        B, T, F_, d = shp.B, shp.T, shp.F, shp.d_ob
        K, D = T * d, F_ * d + self.d_pe
        z = torch.empty((T, B, D), dtype=torch.float32, device=dev)
        mask = torch.empty((B, T), dtype=torch.bool, device=dev)
        times = times.contiguous()
        ts = self.pos_encoder.timescales(dev)
        _lib.call("rd_pe_mask", ctypes.byref(shp), ops._ptr(times), ops._ptr(lengths), ops._ptr(ts), ops._ptr(z), ops._ptr(mask),
                  ops._stream())
        l1, l2 = self.ob_propagation, self.ob_propagation_layer2
        pe1 = edge_dropout_of(self)
        X = ops.obs_embed(src, self.R_u, shp, p_drop, seed).view(B * F_, K)
        V = ops.linear(X, l1.lin_value.weight, l1.lin_value.bias, act=1).view(B, F_, K)
        H = ops.linear(X, l1.increase_dim.weight, l1.increase_dim.bias, exact=True).view(B, F_, T * 32)   # edge scores -> top-K: exact fp32
        p_t = z[:, :, F_ * d:].permute(1, 0, 2).contiguous()                       # [B,T,16]: layout only
        y1, ei2, alpha1 = ops.graph_beta(V, H, l1.map_weights, p_t, g["edge_index"], g["edge_weights"].view(1, -1), d,
                                         alpha_grad=self.compute_distance, p_drop=pe1, seed=seed)
        _, ssum2 = ops.edge_softmax_list_batched(ei2, alpha1, F_, norm_row=1)
        y2 = ops.linear(y1.reshape(B * F_, K), l2.lin_value.weight, l2.lin_value.bias, act=1).view(B, F_, K)
        z = ops.rows_to_tokens(y2, ssum2, z, shp)
        if self.compute_distance:
            distance = ops.structure_distance(alpha1.t().contiguous())
        else:
            distance = torch.zeros((), dtype=torch.float32, device=dev)
        return z, mask, distance

    def forward(self, src, static, times, lengths):
        """src [T,B,2F] (values | observation mask), static [B,d_static] or None, times [T,B],
        lengths [B] -> (logits [B,C], distance 0-d, None)   -- code/models_rd.py:278-387."""
        maxlen, batch_size = src.shape[0], src.shape[1]
        if not src.is_cuda:
            raise _lib.RaindropHipError("Raindrop_v2 runs on a ROCm device only; move inputs with .cuda()")
        dev = src.device
        g = self._graph(dev)
        shp = _lib.shape(batch_size, maxlen, self.d_inp, self.d_ob, d_pe=self.d_pe, nhead=self.nhead,
                         nhid=self.nhid, d_static=self.d_static if self.static else 0,
                         n_classes=self.n_classes, max_len=self.max_len)
        if maxlen != self.max_len:
            raise _lib.RaindropHipError("src.shape[0] (%d) must equal max_len (%d): lin_value is "
                                        "Linear(max_len*d_ob, .)" % (maxlen, self.max_len))
        # the whole training step as two hipGraphs behind this surface (the default; RD_MODULE_GRAPH=0 / self.graph_step = False: off;
        # raindrop_amd/graph_module.py): training calls only, the loss and the optimizer stay the caller's
        if graph_module.enabled(self):
            out = graph_module.forward(self, src, static, times, lengths)
            if out is not None:
                return out, torch.zeros((), dtype=torch.float32, device=dev), None
        p_drop = float(self.dropout.p) if self.training else 0.0
        self._drop_calls += 1
        seed = self.forward_seed(self._drop_calls)
        lengths = lengths.to(device=dev, dtype=torch.int64)
        if self.use_beta:
            z, mask, distance = self._sensor_stage_beta(src.float(), times.float(), lengths, shp, p_drop, seed, g)
        else:
            z, mask = ops.sensor_stage(
                src.float(), times.float(), lengths, self.pos_encoder.timescales(dev), g["ssum"], self.R_u,
                self.ob_propagation.lin_value.weight, self.ob_propagation.lin_value.bias,
                self.ob_propagation_layer2.lin_value.weight, self.ob_propagation_layer2.lin_value.bias, shp,
                p_drop, seed, coef_p=coef_dropout_of(self), edges=(g["edge_index"], g["edge_weights"]))
            # coefficient dropout (training mode): one keep decision per (sample, layer, edge) under this forward's seed -- the
            # aggregate scale ssum[f] becomes a per-(sample, layer, sensor) table (ops.coef_table); the returned structure is untouched.
            # every sample returns the same edge scores on this branch: cdist of equal columns, exactly 0
            distance = torch.zeros((), dtype=torch.float32, device=dev)
        # ---- temporal stage: nn.TransformerEncoder semantics on the HIP kernels (K2/K3) ----------
        r_out = z
        for i, layer in enumerate(self.transformer_encoder.layers):
            named = dict(layer.named_parameters())
            r_out = ops.encoder_layer(r_out, mask, shp, i, p_drop, seed, [named[n] for n in ops.ENC_PARAM_NAMES])
        # ---- masked mean over time + static embedding + classifier head (K5) ---------------------
        if static is not None:
            emb = ops.linear(static.float(), self.emb.weight, self.emb.bias)
            agg = ops.masked_mean(r_out, mask, lengths, shp)
            output = torch.cat([agg, emb], dim=1)                      # code/models_rd.py:384
        else:
            output = ops.masked_mean(r_out, mask, lengths, shp)
        hid = ops.linear(output, self.mlp_static[0].weight, self.mlp_static[0].bias, act=1)
        output = ops.linear(hid, self.mlp_static[2].weight, self.mlp_static[2].bias)
        return output, distance, None
