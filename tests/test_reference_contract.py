"""CPU: install() against the contract of the REAL reference class, as recorded in tests/golden/cgic_contract.npz.

The GPU tests exercise install() on a CGIC-shaped stub; this one rebuilds the real 130 M-parameter `CGIC`
(CGIC/models/model.py) as tests/golden/make_golden_contract.py recorded it from the reference -- every state_dict key at its
shape (meta tensors: nothing is allocated), and at the places install() works on, modules of the kinds the real model has
there, with its quantiser's initial weights and counters -- and checks the attribute contract install() relies on, that
install() runs on it without launching anything, keeps every state_dict key and shape, and points the router target at the
drop-in.  The generator ran install() on the real class itself before writing the fixture."""
import importlib
import json
from collections import OrderedDict

import torch


class _CGICStandIn(torch.nn.Module):
    """the module tree of the recorded model; encode / decode / compress exist (install() replaces compress)"""

    def encode(self, x):
        raise NotImplementedError

    def decode(self, quant):
        raise NotImplementedError

    def compress(self, x):
        raise NotImplementedError


def _stand_in(g, facts):
    names = [str(n) for n in g["sd_names"]]
    shapes = {n: tuple(int(d) for d in s if d >= 0) for n, s in zip(names, g["sd_shapes"])}
    model = _CGICStandIn()

    def owner(path):
        m = model
        for p in path:
            if p not in m._modules:
                m.add_module(p, torch.nn.Module())
            m = m._modules[p]
        return m

    # the places install() works on: modules of the recorded kinds, real tensors where it reads values
    q = owner(["quantize"])
    q.n_e, q.e_dim, q.beta, q.legacy = facts["n_e"], facts["e_dim"], facts["beta"], facts["legacy"]
    q.embedding = torch.nn.Embedding(facts["n_e"], facts["e_dim"])
    q.embedding.weight.data.copy_(torch.from_numpy(g["quantize_weight"]))
    q.embedding_counter = torch.nn.ParameterDict(OrderedDict(
        (str(k), torch.nn.Parameter(torch.full(shapes[f"quantize.embedding_counter.{k}"], float(v)), requires_grad=False))
        for k, v in zip(g["counter_keys"], g["counter"])))
    for name, c in facts["convs"].items():
        assert c["type"] == "Conv2d"
        setattr(model, name, torch.nn.Conv2d(c["in_channels"], c["out_channels"], tuple(c["kernel_size"]), bias=c["bias"]))
    for name, p in facts["decoder_pools"].items():
        assert p["type"] == "AvgPool2d"
        owner(["decoder"]).add_module(name, torch.nn.AvgPool2d(p["kernel_size"], p["stride"], p["padding"]))
    for name in ("entropy_calculation_p8", "entropy_calculation_p16"):
        owner([name])
    owner(["encoder"]).router_config = facts["router_config"]
    # everything else: the recorded entries at their shapes
    done = set(model.state_dict())
    for n, is_param in zip(names, g["sd_is_param"]):
        if n in done:
            continue
        *path, leaf = n.split(".")
        t = torch.empty(shapes[n], device="meta")
        if is_param:
            owner(path).register_parameter(leaf, torch.nn.Parameter(t))
        else:
            owner(path).register_buffer(leaf, t)
    return model


def _instantiate_from_config(config):
    module, cls = config["target"].rsplit(".", 1)
    return getattr(importlib.import_module(module), cls)(**config.get("params", dict()))


def test_install_on_the_real_cgic_class(golden):
    import control_gic_amd as cg
    g = golden("cgic_contract")
    facts = json.loads(str(g["facts"]))

    # ---- the attribute contract install() / compress_batch() rely on (model.py:42-60, 99-117; vqvae_blocks.py:354-355)
    assert facts["quantize_type"] == "VectorQuantize2" and (facts["n_e"], facts["e_dim"]) == (1024, 4) and "beta" in facts
    assert facts["legacy"] is True
    assert g["quantize_weight"].shape == (1024, 4) and len(g["counter_keys"]) == 1024
    assert list(g["counter_keys"][:4]) == ["0", "1", "10", "100"]                 # ParameterDict sorts plain-dict keys as strings
    rc = facts["router_config"]
    assert rc["target"].endswith("TripleGrainFixedEntropyRouter") and {"coarse_grain_ratio", "medium_grain_ratio"} <= set(rc["params"])
    assert facts["entropy_types"] == ["Entropy", "Entropy"]
    qc, pqc = facts["convs"]["quant_conv"], facts["convs"]["post_quant_conv"]
    assert qc["type"] == "Conv2d" and qc["kernel_size"] == [1, 1] and qc["in_channels"] == 4
    assert pqc["type"] == "Conv2d" and pqc["kernel_size"] == [1, 1]
    assert facts["callables"] == ["encode", "decode", "compress"]

    model = _stand_in(g, facts).eval()
    keys = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert keys == {str(n): tuple(int(d) for d in s if d >= 0) for n, s in zip(g["sd_names"], g["sd_shapes"])}
    q = model.quantize
    emb = q.embedding.weight.detach().clone()
    assert q.embedding_counter["7"].item() == 42.0                              # (set before the codes below were recorded)

    cg.install(model)                                                           # CPU: nothing is launched

    assert isinstance(model.quantize, cg.VectorQuantize2) and isinstance(model.entropy_calculation_p8, cg.Entropy)
    assert model.encoder.router_config["target"] == "control_gic_amd.router.TripleGrainFixedEntropyRouter"
    assert model.encoder.router_config["params"]["per_image"] is False         # the reference's batch semantics stay the default
    r = _instantiate_from_config(model.encoder.router_config)
    assert isinstance(r, cg.TripleGrainFixedEntropyRouter) and r.per_image is False
    after = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert after == keys, (set(after) ^ set(keys))                              # same keys, same shapes: checkpoints keep loading
    assert torch.equal(model.quantize.embedding.weight, emb) and model.quantize.embedding_counter["7"].item() == 42.0
    assert list(model.quantize.embedding_counter)[:4] == ["0", "1", "10", "100"]
    # the table HuffmanCoding(model.quantize.embedding_counter) is built from, in the reference's order (inference.py:137-139):
    # the codes the reference's own HuffmanCoding built from the same counters
    h = cg.HuffmanCoding(model.quantize.embedding_counter)
    assert h.codes == {int(k): str(c) for k, c in zip(g["code_keys"], g["codes"])}
