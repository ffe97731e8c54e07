"""Conditional generation, the parts that need no GPU: the tri-state codes of (given, given_mask) and the requests the mode classes refuse
before any device work."""
import pytest
import torch

CPU = torch.device("cpu")


def config(P=8, tracks=("Drums", "Piano", "Guitar")):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 24, "highest": 24 + P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def params(mode, enc="Pass", enc_hidden=None, gen="NADE"):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": enc, "num_hidden": enc_hidden},
            "generator": {"type": gen, "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": [16]}}


def test_given_codes_broadcast_track_pitch_and_full_masks():
    from multinn_amd.common import given_codes, given_tracks, GIVEN_FREE
    B, S, P, M = 2, 3, 4, 3
    g = torch.randint(0, 4, (B, S, P, M), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    on = (g != 0).to(torch.uint8)
    # [M]: whole tracks
    c = given_codes(g, torch.tensor([True, False, True]))
    assert c.dtype == torch.uint8 and c.shape == (B, S, P, M) and c.is_contiguous()
    assert torch.equal(c[..., 0], on[..., 0]) and torch.equal(c[..., 2], on[..., 2]) and bool((c[..., 1] == GIVEN_FREE).all())
    assert given_tracks(torch.tensor([True, False, True]), (B, S, P, M)) == ([True, False, True], [True, False, True])
    # [P, M]: pitch ranges
    pm = torch.zeros(P, M, dtype=torch.bool)
    pm[1:3, 1] = True
    c = given_codes(g, pm)
    assert torch.equal(c[:, :, 1:3, 1], on[:, :, 1:3, 1])
    assert bool((c[:, :, 0, :] == GIVEN_FREE).all()) and bool((c[..., 0] == GIVEN_FREE).all())
    assert given_tracks(pm, (B, S, P, M)) == ([False, False, False], [False, True, False])
    # the full shape
    full = torch.rand(B, S, P, M, generator=torch.Generator().manual_seed(1)) < 0.4
    c = given_codes(g, full)
    assert torch.equal(c[full], on[full]) and bool((c[~full] == GIVEN_FREE).all())
    # nonzero means 1; no mask = every cell given
    assert set(torch.unique(c[full]).tolist()) <= {0, 1}
    assert torch.equal(given_codes(g, None), on)
    assert given_tracks(None, (B, S, P, M)) == ([True] * M, [True] * M)
    # a track masked over every cell of a full-shape mask is whole
    full2 = torch.zeros(B, S, P, M, dtype=torch.bool)
    full2[..., 2] = True
    full2[0, 0, 0, 0] = True
    assert given_tracks(full2, (B, S, P, M)) == ([False, False, True], [True, False, True])


def test_given_codes_bad_shapes_raise_value_error():
    from multinn_amd.common import given_codes, given_tracks
    g = torch.zeros(2, 3, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        given_codes(g, torch.ones(4, dtype=torch.bool))                 # [P] alone does not broadcast over M
    with pytest.raises(ValueError):
        given_codes(g, torch.ones(5, 3, dtype=torch.bool))              # wrong P
    with pytest.raises(ValueError):
        given_codes(g, torch.ones(3, dtype=torch.uint8))                # not bool
    with pytest.raises(ValueError):
        given_codes(g[0], torch.ones(3, dtype=torch.bool))              # not 4-D
    with pytest.raises(ValueError):
        given_codes(g.float(), torch.ones(3, dtype=torch.bool))         # not u8
    with pytest.raises(ValueError):
        given_codes(g, torch.ones(3, dtype=torch.bool), shape=(2, 4, 4, 3))
    with pytest.raises(ValueError):
        given_tracks(torch.ones(2, dtype=torch.bool), (2, 3, 4, 3))


@pytest.mark.parametrize("mode", ["joint", "composer", "jamming", "feedback", "feedback-rnn"])
def test_dbn_encoders_refuse_conditioning(mode):
    from multinn_amd import MultINN
    m = MultINN(config(), params(mode, enc="DBN", enc_hidden=[6]), mode=mode, device=CPU)
    with pytest.raises(NotImplementedError):
        m.generate(4, given=torch.zeros(2, 4, 8, 3, dtype=torch.uint8), given_mask=torch.tensor([True, False, False]))


def test_rbm_generators_refuse_partial_masks():
    from multinn_amd import MultINN
    given = torch.zeros(2, 4, 8, 3, dtype=torch.uint8)
    pm = torch.zeros(8, 3, dtype=torch.bool)
    pm[:4, 0] = True
    for mode in ("jamming", "feedback"):
        m = MultINN(config(), params(mode, gen="RBM"), mode=mode, device=CPU)
        with pytest.raises(NotImplementedError):
            m.generate(4, given=given, given_mask=pm)
    # joint with an RBM generator: any given cell
    m = MultINN(config(), params("joint", gen="RBM"), mode="joint", device=CPU)
    with pytest.raises(NotImplementedError):
        m.generate(4, given=given, given_mask=torch.tensor([True, False, False]))
    with pytest.raises(ValueError):
        m.generate(4, given_mask=torch.tensor([True, False, False]))    # a mask without given


def test_generate_signatures_take_given():
    import inspect
    from multinn_amd.modes import MultINNJoint, MultINNComposer, MultINNJamming, MultINNFeedback, MultINNFeedbackRnn, MultINNCore
    from multinn_amd.generators import RnnEstimator, RnnNade
    for cls in (MultINNJoint, MultINNComposer, MultINNJamming, MultINNFeedback, MultINNFeedbackRnn):
        ps = inspect.signature(cls.generate).parameters
        assert ps["given"].default is None and ps["given_mask"].default is None
    assert "given" in inspect.signature(MultINNCore.sampler).parameters
    assert inspect.signature(RnnEstimator.generate).parameters["given"].default is None
    assert inspect.signature(RnnNade.sample_single).parameters["given"].default is None
