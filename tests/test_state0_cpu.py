"""The learned initial LSTM state (`learn_zero_state`, rnn.py:18-24, 139-143, 214-217) without a device: constructor, variable layout,
parameter counts, checkpoints and what is refused."""
import pytest
import torch

from multinn_amd.common import RNN, ParamStore


def _nade(**kw):
    from multinn_amd import RnnNade
    g = RnnNade(440, 256, [512, 256], device="cpu", seed=23, **kw)
    g._materialize(440)
    return g


def test_rnn_constructs_and_declares_c0_behind_all_cell_variables():
    r = RNN([512, 256], learn_zero_state=True)
    assert r.learn_zero_state and not RNN([512, 256]).learn_zero_state
    st = ParamStore("cpu")
    r.declare(st, 440, torch.Generator().manual_seed(1))
    names = st.names()
    assert names == ["rnn/cell_0/kernel", "rnn/cell_0/bias", "rnn/cell_1/kernel", "rnn/cell_1/bias", "rnn/cell_0/c0", "rnn/cell_1/c0"]
    st.materialize()
    assert tuple(st["rnn/cell_0/c0"].shape) == (1, 512) and tuple(st["rnn/cell_1/c0"].shape) == (1, 256)
    assert float(st["rnn/cell_0/c0"].abs().max()) == 0.0 and float(st["rnn/cell_1/c0"].abs().max()) == 0.0


def test_zero_state_tiles_c0_and_its_tanh():
    r = RNN([64, 32], learn_zero_state=True)
    st = ParamStore("cpu")
    r.declare(st, 8, torch.Generator().manual_seed(1))
    st.materialize()
    st["rnn/cell_0/c0"].copy_(torch.linspace(-1, 1, 64).view(1, 64))
    s = r.zero_state(5)
    assert len(s) == 2 and tuple(s[0][0].shape) == (5, 64) and tuple(s[1][1].shape) == (5, 32)
    assert torch.equal(s[0][0], st["rnn/cell_0/c0"].expand(5, 64)) and torch.equal(s[0][1], torch.tanh(st["rnn/cell_0/c0"]).expand(5, 64))
    assert float(s[1][0].abs().max()) == 0.0 and float(s[1][1].abs().max()) == 0.0
    plain = RNN([64, 32])
    plain.declare(ParamStore("cpu"), 8, torch.Generator().manual_seed(1))
    plain.store.materialize()
    assert all(float(c.abs().max()) == 0.0 and float(h.abs().max()) == 0.0 for c, h in plain.zero_state(3))


def test_attn_length_still_raises_with_its_own_message():
    for kw in (dict(attn_length=1), dict(attn_length=1, learn_zero_state=True)):
        with pytest.raises(NotImplementedError, match="AttentionCellWrapper") as e:
            RNN([64], **kw)
        assert "attn_length" in str(e.value) and "learn_zero_state" not in str(e.value)


def test_parameter_counts_and_flag_off_layout_unchanged():
    off, on = _nade(), _nade(learn_zero_state=True)
    assert off.store.theta.numel() == 3143352
    assert on.store.theta.numel() == 3144120                 # + 512 + 256
    assert off.store.names() == ["rnn/cell_0/kernel", "rnn/cell_0/bias", "rnn/cell_1/kernel", "rnn/cell_1/bias", "nade/w_enc", "nade/w_dec",
                                 "dense/kernel", "dense/bias"]
    assert [n for n in on.store.names() if not n.endswith("/c0")] == off.store.names()
    assert on.store.names()[4:6] == ["rnn/cell_0/c0", "rnn/cell_1/c0"]
    for n in off.store.names():                              # zeros_init draws nothing: every other weight is the flag-off model's
        assert tuple(on.store[n].shape) == tuple(off.store[n].shape) and torch.equal(on.store[n], off.store[n]), n
    assert not off.learn_zero_state and on.learn_zero_state and off._state0(4) is None
    assert [tuple(c.shape) for c, _ in on._state0(4)] == [(4, 512), (4, 256)]


def test_flag_reaches_every_generator_class():
    from multinn_amd import RnnMultiNADE, RnnRBM
    m = RnnMultiNADE(8, 16, [64, 32], tracks=list("ab"), device="cpu", learn_zero_state=True)
    m._materialize(16)
    r = RnnRBM(16, 16, [64, 32], device="cpu", learn_zero_state=True)
    r._materialize(16)
    for g in (m, r):
        assert g._rnn.learn_zero_state and "rnn/cell_1/c0" in g.store.names()
    assert r.store.names().index("rnn/cell_0/c0") == r.store.names().index("rnn/cell_1/bias") + 1      # ... behind the rnn block, in front of Wuh


def test_state_dict_round_trip_with_nonzero_c0(tmp_path):
    a, b = _nade(learn_zero_state=True), _nade(learn_zero_state=True)
    a.store["rnn/cell_0/c0"].copy_(torch.linspace(-0.5, 0.5, 512).view(1, 512))
    a.store["rnn/cell_1/c0"].fill_(0.25)
    a.save(ckpt_dir=str(tmp_path))
    assert b.load(ckpt_dir=str(tmp_path))
    assert torch.equal(b.store["rnn/cell_0/c0"], a.store["rnn/cell_0/c0"]) and float(b.store["rnn/cell_1/c0"].min()) == 0.25
    assert torch.equal(a.store.theta, b.store.theta)
    with pytest.raises(ValueError):                          # a flag-off model does not take the checkpoint of a flag-on one
        _nade().store.load_state_dict(a.store.state_dict())


def _config_params(mode):
    config = {"data": {"pitch_range": {"lowest": 24, "highest": 32}, "instruments": ["a", "b"], "beat_resolution": 4},
              "training": {"num_pixels": 1, "random_seed": 3}, "model_name": "m"}
    params = {"mode": mode, "keep_prob": 0.9, "tune_encoder": False, "encoder": {"type": "Pass", "num_hidden": [8]},
              "generator": {"type": "NADE", "num_hidden": 16, "num_hidden_rnn": [64, 32], "learn_zero_state": True,
                            "feedback": {"num_hidden": 16, "num_hidden_rnn": [32]}}}
    return config, params


@pytest.mark.parametrize("mode", ["feedback", "feedback-rnn"])
def test_feedback_modes_refuse_the_flag(mode):
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd.modes import MultINN
    config, params = _config_params(mode)
    with pytest.raises(MnnUnsupported, match="learn_zero_state"):
        MultINN(config, params, mode=mode, device="cpu")


@pytest.mark.parametrize("mode", ["joint", "jamming", "composer"])
def test_other_modes_hand_the_flag_to_their_generators(mode):
    from multinn_amd.modes import MultINN
    config, params = _config_params(mode)
    m = MultINN(config, params, mode=mode, device="cpu")
    gens = m.generators if hasattr(m, "generators") else m._generators
    assert gens and all(g.learn_zero_state for g in gens)
    params["generator"]["learn_zero_state"] = False
    m2 = MultINN(config, params, mode=mode, device="cpu")
    assert not any(g.learn_zero_state for g in (m2.generators if hasattr(m2, "generators") else m2._generators))


def test_build_generator_reads_the_flag():
    from multinn_amd.driver import build_generator
    params = {"mode": "joint", "encoder": {"type": "Pass"}, "generator": {"type": "NADE", "num_hidden": 16, "num_hidden_rnn": [64], "learn_zero_state": True}}
    assert build_generator(params, 8, 2).learn_zero_state
    params["generator"].pop("learn_zero_state")
    assert not build_generator(params, 8, 2).learn_zero_state
