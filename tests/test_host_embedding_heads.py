"""CPU checks of the embedding-level exit heads' fit path: the names ``state_dict(cfg, embedding_exits=True)`` produces for all four fit
classes, what the Python surface still refuses, and the C entry point ``ee_embedding_inputs`` (declared, plain C, exported)."""
import os
import re

import numpy as np
import pytest

from .conftest import ROOT
from .fit_util import _HostTensor, compiles_as_c, exported_symbols

ALL_KINDS = ["vision_avg", "text_avg", "text_visual_concat", 1, 2]
GAP = ["text_avg", 1, 4]                                    # one kind of three: the names must not count kinds that are absent
EMB_NAME = {"vision_avg": "vision_exit_embeddings", "text_avg": "text_exit_embeddings", "text_visual_concat": "concat_exit_embeddings"}
FITS = ["HeadFit", "MlpHeadFit", "GateFit", "MlpGateFit"]


def _cfg(pkg, exits, fit_name, **more):
    ee = dict(exits=list(exits), encoder_layer_strategy="gate" if "Gate" in fit_name else "ramp",
              exit_head_num_layers=2 if "Mlp" in fit_name else 1)
    return pkg.ModelConfig.tiny(EE_config=ee, **more)


def _host_fit(pkg, fit_name, E, K, H, seed=0):
    """A fit object of the class with host arrays standing in for its device tensors -> (fit, {tensor suffix: (E, ...) array})"""
    rng = np.random.default_rng(seed)
    a = {"out_proj.weight": rng.standard_normal((E, K, H)).astype(np.float32), "out_proj.bias": rng.standard_normal((E, K)).astype(np.float32)}
    w, b = _HostTensor(a["out_proj.weight"]), _HostTensor(a["out_proj.bias"])
    if "Mlp" not in fit_name:
        return getattr(pkg, fit_name)(w, b, None, None, None, None, None, None, 1e-2), a
    a["dense.weight"] = rng.standard_normal((E, H, H)).astype(np.float32)
    a["dense.bias"] = rng.standard_normal((E, H)).astype(np.float32)
    return getattr(pkg, fit_name)(_HostTensor(a["dense.weight"]), _HostTensor(a["dense.bias"]), w, b, None, None, None, None, None, 1e-2), a


def _stems(exits):
    emb = [e for e in ("vision_avg", "text_avg", "text_visual_concat") if e in exits]                 # the reference's order
    n_enc = len([e for e in exits if isinstance(e, int)])
    return [f"layoutlmv3.{EMB_NAME[e]}" for e in emb] + [f"layoutlmv3.encoder.early_exits.{k}" for k in range(n_enc)]


@pytest.mark.parametrize("exits", [ALL_KINDS, GAP], ids=["all_kinds", "gap"])
@pytest.mark.parametrize("fit_name", FITS)
def test_state_dict_names_every_head_of_the_configuration(pkg, fit_name, exits):
    cfg = _cfg(pkg, exits, fit_name)
    W = pkg.synth.make_weights(cfg, seed=1)
    K = 2 if "Gate" in fit_name else cfg.num_labels
    stems = _stems(exits)
    fit, arrays = _host_fit(pkg, fit_name, len(stems), K, cfg.hidden_size)
    sd = fit.state_dict(cfg, embedding_exits=True)
    assert set(sd) == {k for k in W if "exit" in k}, set(sd) ^ {k for k in W if "exit" in k}
    assert len(sd) == len(stems) * len(arrays)
    for i, stem in enumerate(stems):                                    # row i of the fit lands under the i-th exit's name
        for suffix, a in arrays.items():
            v = sd[f"{stem}.{suffix}"]
            assert v.shape == W[f"{stem}.{suffix}"].shape and v.dtype == np.float32 and v.flags["C_CONTIGUOUS"], (stem, suffix)
            assert np.array_equal(v, a[i]), (stem, suffix)
        if "Gate" in fit_name:
            assert sd[f"{stem}.out_proj.weight"].shape == (2, cfg.hidden_size)


@pytest.mark.parametrize("fit_name", FITS)
def test_refusals(pkg, fit_name):
    cfg = _cfg(pkg, ALL_KINDS, fit_name)
    K, H = (2 if "Gate" in fit_name else cfg.num_labels), cfg.hidden_size
    five, _ = _host_fit(pkg, fit_name, 5, K, H)
    two, _ = _host_fit(pkg, fit_name, 2, K, H)
    with pytest.raises(ValueError, match="3 embedding-level \\+ 2 encoder exits"):        # both counts are named
        two.state_dict(cfg, embedding_exits=True)
    for fit in (five, two):                                             # the default call keeps its refusal, whatever the fit's shape
        with pytest.raises(ValueError, match="embedding-level"):
            fit.state_dict(cfg)
    # without embedding exits in the configuration the flag changes nothing
    plain = _cfg(pkg, [1, 2], fit_name)
    assert sorted(two.state_dict(plain, embedding_exits=True)) == sorted(two.state_dict(plain))
    with pytest.raises(ValueError, match="the fit is"):
        five.state_dict(plain, embedding_exits=True)
    # embedding exits alone: allowed with the flag
    only = _cfg(pkg, ["vision_avg", "text_avg"], fit_name)
    assert {k.split(".")[1] for k in two.state_dict(only, embedding_exits=True)} == {"vision_exit_embeddings", "text_exit_embeddings"}


def test_beit_is_refused(pkg):
    ee = dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=1)
    cfg = pkg.ModelConfig.dit_tiny(EE_config=ee)
    fit, _ = _host_fit(pkg, "HeadFit", 2, cfg.num_labels, cfg.hidden_size)
    assert fit.state_dict(cfg)                                          # the encoder heads of a DiT handle are fitted as before
    with pytest.raises(ValueError, match="BEiT"):
        fit.state_dict(cfg, embedding_exits=True)

    class _Engine:
        pass
    eng = _Engine()
    eng.cfg = cfg
    with pytest.raises(ValueError, match="BEiT"):
        pkg.collect_exit_features(eng, [], embedding_exits=True)
    with pytest.raises(ValueError, match="BEiT"):
        pkg.collect_distill_features(eng, [], embedding_exits=True)
    with pytest.raises(ValueError, match="BEiT"):
        pkg.collect_embedding_features(eng, [])


def test_collectors_keep_their_default_refusal(pkg):
    class _Engine:
        pass
    eng = _Engine()
    eng.cfg = _cfg(pkg, ALL_KINDS, "HeadFit")
    with pytest.raises(ValueError, match="embedding-level"):
        pkg.collect_exit_features(eng, [])
    with pytest.raises(ValueError, match="embedding-level"):
        pkg.collect_distill_features(eng, [])


def test_entry_point_is_declared_mirrored_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert "ee_embedding_inputs" in set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    assert len(pkg.capi.SYMBOLS["ee_embedding_inputs"][1]) == 13
    assert "ee_embedding_inputs" in exported_symbols(pkg.capi.lib_path())
    assert pkg.collect_embedding_features is pkg.heads.collect_embedding_features
    assert callable(pkg.EarlyExitEngine.embedding_inputs)


def test_prototype_compiles_as_c():
    compiles_as_c('    int (*a)(ee_handle*, const int64_t*, const int64_t*, const int64_t*, const float*, const int64_t*, const int64_t*, int32_t, int32_t,'
                  ' float*, float*, float*, void*) = ee_embedding_inputs;\n'
                  '    (void)a;\n'
                  '    return 0;\n')
