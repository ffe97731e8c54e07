"""The composer-mode LSTM-RBM (generator type `MultiRBM`) without a GPU: construction and variable layout, where the type is accepted, the
two C-ABI additions in header / loader / library, the grouped kernels' build properties, and the ops wrappers' host checks."""
import os
import re
import subprocess

import pytest
import torch

from test_modes_cpu import config, params

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("mnn_rbm_gibbs_multi", "mnn_rbm_free_energy_multi")


def test_composer_mode_builds_one_multirbm_with_the_specified_variables():
    from multinn_amd import modes, RnnMultiRBM, RnnRBM
    P, tracks, Hn, units = 8, ("Drums", "Piano", "Guitar"), 16, (64, 32)
    p = params("composer", gen="MultiRBM", Hn=Hn, units=units)
    m = modes.MultINN(config(P, tracks), p, mode="composer", device=CPU)
    assert m.generator_type == "MultiRBM" and len(m.generators) == 1 and len(m.encoders) == 3
    g = m.generators[0]
    assert isinstance(g, RnnMultiRBM) and g.num_dims == P and g.tracks == list(tracks) and g.num_tracks == 3 and g.name == "rnn-multirbm"
    assert g.k == 10 and g.internal_bias is True and g.bias_mode == "conditional" and g.seed == 23
    g._materialize(P * 3)
    M, R = 3, units[-1]
    want = []
    for i in range(M):
        want += [(f"rbm_{i}/W", (P, Hn)), (f"rbm_{i}/bv", (1, P)), (f"rbm_{i}/bh", (1, Hn))]
    want += [("rnn/cell_0/kernel", (P * M + units[0], 4 * units[0])), ("rnn/cell_0/bias", (4 * units[0],)),
             ("rnn/cell_1/kernel", (units[0] + units[1], 4 * units[1])), ("rnn/cell_1/bias", (4 * units[1],)),
             ("Wuh", (R, M * Hn)), ("Wuv", (R, M * P))]
    assert [(n, tuple(g.store[n].shape)) for n in g.store.names()] == want
    # per-track RBM m draws from the generator's RNG in track order: the first RBM's weights are RnnRBM's of the same seed
    one = RnnRBM(num_dims=P, num_hidden=Hn, num_hidden_rnn=list(units), device=CPU, seed=23)
    one._materialize(P * 3)
    assert torch.equal(g.store["rbm_0/W"], one.store["rbm/W"])
    assert not torch.equal(g.store["rbm_1/W"], g.store["rbm_0/W"])
    # k from params; learn_zero_state declares c0 inside the rnn block
    p2 = params("composer", gen="MultiRBM", Hn=Hn, units=units)
    p2["generator"].update(k=3, learn_zero_state=True)
    g2 = modes.MultINNComposer(config(P, tracks), p2, device=CPU).generators[0]
    g2._materialize(P * 3)
    assert g2.k == 3 and g2.learn_zero_state
    names = g2.store.names()
    c0 = [n for n in names if "c0" in n]
    assert c0 and all(names.index("rbm_2/bh") < names.index(n) < names.index("Wuh") for n in c0)
    z = g2.zero_state(4)
    assert len(z.b_enc) == 3 and len(z.b_dec) == 3 and tuple(z.b_enc[1].shape) == (4, Hn) and tuple(z.b_dec[2].shape) == (4, P)


@pytest.mark.parametrize("mode", ["joint", "jamming", "feedback", "feedback-rnn"])
def test_multirbm_is_refused_outside_composer_mode(mode):
    from multinn_amd import modes
    with pytest.raises(ValueError, match="MultiRBM"):
        modes.MultINN(config(), params(mode, gen="MultiRBM", feedback=[32, 16]), mode=mode, device=CPU)
    from multinn_amd import driver
    with pytest.raises(ValueError):
        driver.build_generator(dict(params("joint", gen="MultiRBM")), 8, 3)


def test_generator_argument_checks():
    from multinn_amd import RnnMultiRBM
    with pytest.raises(ValueError):
        RnnMultiRBM(num_dims=4, num_hidden=8, num_hidden_rnn=[8], tracks=[str(i) for i in range(9)], device=CPU)
    with pytest.raises(ValueError):
        RnnMultiRBM(num_dims=4, num_hidden=8, num_hidden_rnn=[8], tracks=[], device=CPU)


def test_new_symbols_in_header_loader_and_library():
    from multinn_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert s in _lib.SIGNATURES, s
    assert re.search(r"#define\s+MNN_ABI_VERSION\s+124\b", header) and _lib.ABI_VERSION == 124
    lib = _lib.load()
    assert lib.mnn_version() == 124
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    exported = set(re.findall(r"\bT (mnn_[a-z0-9_]+)", out))
    assert set(NEW_SYMBOLS) <= exported
    assert "rbm_multi.hip" in build.SOURCES


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_grouped_kernels_use_no_scratch_and_the_matrix_cores(tmp_path):
    from multinn_amd import build
    out = str(tmp_path / "rbm_multi.s")
    subprocess.check_call([HIPCC] + build.flags_for("rbm_multi.hip") + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "rbm_multi.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = {m.group(1): int(m.group(2))
             for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    # the three chain kernel templates of rbm_chain.h over the job-table block: (4 LDS + 1 matrix-core + 1 streaming) x given x tempered
    for nm, count in (("rbm_gibbs_lds_kernel", 16), ("rbm_gibbs_mfma_kernel", 4), ("rbm_gibbs_stream_kernel", 4), ("rbm_free_energy_multi_kernel", 1)):
        hit = {k: v for k, v in sizes.items() if nm in k}
        assert len(hit) == count and all(v == 0 for v in hit.values()), (nm, hit)
    chain = [k for k in sizes if "rbm_gibbs_" in k]
    assert len(chain) == 24 and all("GibbsTableArgs" in k for k in chain), chain      # and no single-job kernel: those are rbm.hip's
    seen = 0
    for body in re.split(r"\n(?=_Z\w+:)", text):
        if re.match(r"_Z\w*rbm_gibbs_mfma_kernel", body):
            seen += 1
            assert "v_mfma_f32_32x32x2_f32" in body and "scratch_" not in body, body[:70]
    assert seen == 4


def _job(N=6, D=5, Hn=4, **kw):
    j = dict(v0=torch.zeros((N, D), dtype=torch.uint8), W=torch.zeros((D, Hn)), bh=torch.zeros((N, Hn)), bv=torch.zeros((N, D)), seed=1,
             p_v=torch.zeros((N, D)), v_out=torch.zeros((N, D), dtype=torch.uint8))
    j.update(kw)
    return j


def _fe_job(N=6, D=5, Hn=4, **kw):
    j = dict(v=torch.zeros((N, D), dtype=torch.uint8), W=torch.zeros((D, Hn)), bh=torch.zeros((N, Hn)), bv=torch.zeros((N, D)), F=torch.zeros(N))
    j.update(kw)
    return j


def test_ops_wrappers_refuse_bad_job_lists_before_any_device_work():
    """Host tensors throughout: a wrapper that reached the device would raise MnnError (no CPU path), not ValueError."""
    from multinn_amd import ops
    for bad in ([], [_job() for _ in range(9)],
                [_job(), _job(N=7)],                                              # mismatched rows
                [_job(), _job(Hn=3)],                                             # mismatched hidden width
                [_job(), _job(W=torch.zeros((5, 4), dtype=torch.float64))],
                [_job(), _job(bh=torch.zeros((6, 8))[:, :4])],                    # another leading dimension
                [_job(), _job(p_v=torch.zeros((6, 10))[:, ::2])],                 # output strides differ from v0's
                [_job(given=torch.zeros((6, 5), dtype=torch.uint8)), _job()]):    # given on some jobs only
        with pytest.raises(ValueError):
            ops.rbm_gibbs_multi(bad, 2)
    with pytest.raises(ValueError):
        g = torch.zeros((6, 5), dtype=torch.uint8)
        ops.rbm_gibbs_multi([_job(given=g), _job(given=g)], 2, seed_step=torch.zeros(1, dtype=torch.int32))
    for bad in ([], [_fe_job() for _ in range(9)], [_fe_job(), _fe_job(N=7)], [_fe_job(), _fe_job(D=6)], [_fe_job(), _fe_job(F=torch.zeros(5))],
                [_fe_job(), _fe_job(p_h=torch.zeros((6, 3)))]):
        with pytest.raises(ValueError):
            ops.rbm_free_energy_multi(bad)
