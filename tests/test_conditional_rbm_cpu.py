"""Conditional generation with RBM generators, the parts that need no GPU: which masks the mode classes accept now that RBM generators run a
clamped Gibbs chain, and the early refusal of a conditional request on a model that does not live on a ROCm device."""
import pytest
import torch

CPU = torch.device("cpu")


def config(P=8, tracks=("Drums", "Piano", "Guitar")):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 24, "highest": 24 + P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def params(mode, gen="RBM"):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
            "generator": {"type": gen, "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": [16]}}


def partial_mask(P=8, M=3):
    pm = torch.zeros(P, M, dtype=torch.bool)
    pm[:4, 0] = True
    return pm


def test_jamming_and_joint_rbm_accept_partial_masks():
    from multinn_amd import MultINN
    from multinn_amd.common import given_tracks
    shape = (2, 4, 8, 3)
    whole, some = given_tracks(partial_mask(), shape)
    assert some[0] and not whole[0]
    for mode in ("jamming", "joint"):
        m = MultINN(config(), params(mode), mode=mode, device=CPU)
        m._refuse_given(whole, some)                                    # no NotImplementedError
        m._refuse_given(*given_tracks(torch.rand(shape) < 0.5, shape))


def test_feedback_rbm_still_refuses_partial_masks():
    from multinn_amd import MultINN
    from multinn_amd.common import given_tracks
    shape = (2, 4, 8, 3)
    for mode in ("feedback", "feedback-rnn"):
        m = MultINN(config(), params(mode), mode=mode, device=CPU)
        with pytest.raises(NotImplementedError):
            m._refuse_given(*given_tracks(partial_mask(), shape))
        m._refuse_given(*given_tracks(torch.tensor([True, False, False]), shape))    # whole tracks: pasted in


@pytest.mark.parametrize("mode,gen", [("jamming", "RBM"), ("joint", "RBM"), ("joint", "NADE"), ("composer", "NADE")])
def test_conditional_request_on_a_cpu_model_fails_early(mode, gen):
    from multinn_amd import MultINN
    from multinn_amd._lib import MnnError
    m = MultINN(config(), params(mode, gen=gen), mode=mode, device=CPU)
    with pytest.raises(NotImplementedError) as e:
        m.generate(4, given=torch.zeros(2, 4, 8, 3, dtype=torch.uint8), given_mask=partial_mask())
    assert isinstance(e.value, MnnError) and "ROCm" in str(e.value)
    with pytest.raises(ValueError):                                     # the format checks come first
        m.generate(4, given=torch.zeros(2, 5, 8, 3, dtype=torch.uint8), given_mask=partial_mask())


def test_rbm_sampling_signatures_take_given():
    import inspect
    from multinn_amd import ops
    from multinn_amd.common import RBM
    from multinn_amd.generators import RnnRBM
    assert inspect.signature(ops.rbm_gibbs).parameters["given"].default is None
    assert inspect.signature(RBM.sample).parameters["given"].default is None
    assert inspect.signature(RnnRBM.sample_single).parameters["given"].default is None
