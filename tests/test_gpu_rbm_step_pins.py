"""The LSTM-RBM step of RnnRBM and RnnMultiRBM, pinned: for eight small cases that reach every branch of build / backward / estimate_nll /
generate, the ordered list of C entries the step calls and SHA-256 digests of its deterministic outputs, both as literals recorded on an
MI355X before the two classes were folded into one implementation -- and the one-track equivalence of the two classes.

The call lists prove that a change of the Python adds, drops or reorders no launch; the digests that the chain ends, conditionals, free
energies, costs, sampling states and samples keep their bits.  Gradients and the loss pass through split-K and atomic reductions and are
not digested: the float64 oracles of test_gpu_multirbm.py / test_gpu_ragged_oracle.py bound them, and the equivalence test below."""
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [6, 3, 5, 1, 4]
SMALL = dict(dims=12, hidden=16, units=[32, 32], B=5, T=6, precision="fp32")
WIDE = dict(dims=12, hidden=20, units=[128, 128], B=8, T=6, precision="bf16")       # Hn + D = 32 < ldo = 64: the padding columns exist
ABC = list("abc")
CASES = {
    "rbm_ragged": dict(SMALL, tracks=None, lengths=LENGTHS, kw=dict(internal_bias=True)),
    "rbm_internal_mode": dict(SMALL, tracks=None, lengths=None, kw=dict(bias_mode="internal")),
    "rbm_learned_state": dict(SMALL, tracks=None, lengths=LENGTHS, kw=dict(internal_bias=False, learn_zero_state=True)),
    "rbm_bf16": dict(WIDE, tracks=None, lengths=None, kw={}),
    "multi_ragged": dict(SMALL, tracks=ABC, lengths=LENGTHS, kw=dict(internal_bias=True)),
    "multi_internal_mode": dict(SMALL, tracks=ABC, lengths=None, kw=dict(bias_mode="internal")),
    "multi_bf16": dict(WIDE, tracks=ABC, lengths=None, kw={}),
    "multi_one_track": dict(SMALL, tracks=["all"], lengths=LENGTHS, kw=dict(internal_bias=True)),
}


def make(case):
    """The case's generator with every variable drawn from a fixed torch.Generator, and its batch (x, y, lengths)."""
    from multinn_amd import RnnRBM, RnnMultiRBM
    c = CASES[case]
    M = len(c["tracks"]) if c["tracks"] else 1
    kw = dict(keep_prob=0.9, k=3, precision=c["precision"], seed=23, **c["kw"])
    g = RnnRBM(c["dims"], c["hidden"], c["units"], **kw) if c["tracks"] is None else RnnMultiRBM(c["dims"], c["hidden"], c["units"], tracks=c["tracks"], **kw)
    g._materialize(c["dims"] * M)
    rng = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        g.store.theta.copy_((torch.rand(g.store.theta.numel(), generator=rng) - 0.5) * 0.5)
    g._packed_step = -1
    dev = g.store.theta.device
    seq = (torch.rand((c["B"], c["T"] + 1, c["dims"] * M), generator=rng) < 0.2).to(torch.uint8).to(dev)
    lengths = None if c["lengths"] is None else torch.tensor(c["lengths"], dtype=torch.int32)
    return g, seq[:, :-1].contiguous(), seq[:, 1:].contiguous(), lengths


def digest(value):
    """SHA-256 of the raw bytes of a tensor, or of a per-track list of tensors in track order."""
    h = hashlib.sha256()
    for t in value if isinstance(value, (list, tuple)) else [value]:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(case, monkeypatch):
    """-> (C entry names in call order, {output: digest}) of a train-mode build, backward, one estimate_nll and one generate."""
    from multinn_amd import ops
    g, x, y, lengths = make(case)
    calls, inner = [], ops.call

    def recording(name, *args):
        calls.append(name)
        return inner(name, *args)
    monkeypatch.setattr(ops, "call", recording)
    g.build(x, y, lengths, True, "train")
    out = {n: digest(getattr(g, n)) for n in ("_outputs", "cond_probs", "free_energy", "cost")}
    g.backward()
    g.check()
    est = g.estimate_nll(y, lengths, num_chains=4, num_betas=8, method="both")
    assert torch.isfinite(est.lower.nll).all() and torch.isfinite(est.upper.nll).all()
    out["nll_lower"], out["nll_upper"] = digest(est.lower.nll), digest(est.upper.nll)
    state = g.steps(x)
    out["b_enc"], out["b_dec"] = digest(state.b_enc), digest(state.b_dec)
    out["samples"] = digest(g.generate(x, 3))
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "call", inner)
    return calls, out


# case -> (C entries in call order, without their "mnn_" prefix, "name*n" for n calls in a row; digests).  Recorded twice, in two processes
# that ran the cases in opposite orders: every call list and every digest came out the same both times, so none had to be dropped.
PINS = {
    "rbm_ragged": (
        "lstm_pack_weights*2 transpose convert2d gemm_tn lstm_seq_fwd dropout_fwd gemm_tn lstm_seq_fwd dropout_fwd gemm_tn rbm_gibbs_stepped rbm_free_energy*2 "
        "weighted_sum log_loss_rows weighted_sum*2 rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn transpose bias_grad*2 transpose gemm_tn*3 dropout_bwd "
        "lstm_seq_bwd gemm_tn dropout_bwd lstm_seq_bwd transpose gemm_tn*2 lstm_unpack_grads_consume transpose gemm_tn*2 lstm_unpack_grads_consume gemm_tn "
        "lstm_seq_fwd gemm_tn lstm_seq_fwd gemm_tn rbm_gibbs_stepped rbm_free_energy*2 weighted_sum log_loss_rows weighted_sum*2 rbm_free_energy rbm_ais "
        "rbm_raise det_lstm_pack*2 lstm_step_det*12 dense_det lstm_step_det*12 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 "
        "dense_det det_lstm_pack*2 lstm_step_det*12 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 "
        "dense_det",
        dict(
            _outputs="ffdc5f26b6c6b2da97ed51466a7c308fecbeb1913dfb76ed46fe9f1f5d920978",
            cond_probs="554f5477606b3190a2ca7a681a6f3c2710614ffc6617a46122e79f8335104c91",
            free_energy="dbd47d04d4d987bfb92604fdbfe1a87b93d622b2373b4503aadaa995755706f2",
            cost="2e8335a1b6562293ef70ad776334d5a581a6015a3b13d2aa56e27a223598192a",
            nll_lower="7e8b4383f4e179d39b777b3e0ead26682b8f93e5fb07fdff42d9ae898f7a104e",
            nll_upper="324a0cb5dfc638451c7d794b1aa23080c6892ade3306f67eb08ac1fffba75631",
            b_enc="1cea84da058586e844f9c8d6525b0189231617ed875b9276e51b1dfabab3cad5",
            b_dec="c133f755a82d9509d67250e35253cedb1a8407126575f150535feb7a4a9bab15",
            samples="5fd4fcbbeaaad02832afaa957d22afcd5d30f8285a6127e5b44f1129595428fb",
        )),
    "rbm_internal_mode": (
        "lstm_pack_weights*2 transpose convert2d gemm_tn lstm_seq_fwd dropout_fwd gemm_tn lstm_seq_fwd dropout_fwd gemm_tn rbm_gibbs_stepped rbm_free_energy*2 "
        "weighted_sum log_loss_rows weighted_sum*2 rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn bias_grad*2 gemm_tn lstm_seq_fwd gemm_tn lstm_seq_fwd "
        "gemm_tn rbm_gibbs_stepped rbm_free_energy*2 weighted_sum log_loss_rows weighted_sum*2 rbm_free_energy rbm_ais rbm_raise det_lstm_pack*2 "
        "lstm_step_det*12 dense_det lstm_step_det*12 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 dense_det det_lstm_pack*2 "
        "lstm_step_det*12 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 dense_det",
        dict(
            _outputs="c9032d9db19db01c7f8f64a5bcc48c5b9a1301d1ebef4c6cf5279f5eee34286e",
            cond_probs="6b5af12fa1919b413825f72f9c207ce95b6834cd9799913fe5a3a22de4771758",
            free_energy="ae9c9ff32e0b5c688185028d5bf053a393344fa6828aac0df97b11535ce812a2",
            cost="ff298e34e1770c541b333c69ffd04f8887a2dc65f16e6b078165d96297bafd05",
            nll_lower="81c6eea575d047cca213345a91d593114640841c771fec5790660390737f825c",
            nll_upper="2442a5fc111963f0874c52752b8d82987cbb2225a2b90bcd91cb0a76920c1c7a",
            b_enc="1cea84da058586e844f9c8d6525b0189231617ed875b9276e51b1dfabab3cad5",
            b_dec="c133f755a82d9509d67250e35253cedb1a8407126575f150535feb7a4a9bab15",
            samples="5fd4fcbbeaaad02832afaa957d22afcd5d30f8285a6127e5b44f1129595428fb",
        )),
    "rbm_learned_state": (
        "lstm_pack_weights*2 transpose convert2d transpose*2 gemm_tn lstm_seq_fwd dropout_fwd gemm_tn lstm_seq_fwd dropout_fwd gemm_tn rbm_gibbs_stepped "
        "rbm_free_energy*2 weighted_sum log_loss_rows weighted_sum*2 rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn transpose*2 gemm_tn*3 dropout_bwd "
        "lstm_seq_bwd gemm_tn dropout_bwd lstm_seq_bwd transpose gemm_tn*2 lstm_unpack_grads_consume transpose gemm_tn*2 lstm_unpack_grads_consume bias_grad*4 "
        "gemm_tn lstm_seq_fwd gemm_tn lstm_seq_fwd gemm_tn rbm_gibbs_stepped rbm_free_energy*2 weighted_sum log_loss_rows weighted_sum*2 rbm_free_energy "
        "rbm_ais rbm_raise det_lstm_pack*2 lstm_step_det*12 dense_det lstm_step_det*12 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 "
        "dense_det det_lstm_pack*2 lstm_step_det*12 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 "
        "dense_det",
        dict(
            _outputs="f288f89500b0b60d293ee9a4f044d1dabd91e4c5420212e14cee7c009d08e0fd",
            cond_probs="993086385a907bb31e43dd1af65c3c244dc4925a8dc4b5d882cb2544f809e075",
            free_energy="ab80a3e0f693b745d17d4b65932316767e167034ed8640115313186d9618e5a2",
            cost="e2bccfdd6ad5bbebf4ccd2533d0d399e33731cc5fc9826b3a09ca5c5260af58a",
            nll_lower="315fe9d1ac4311aff2c963064559c77752cd8186e673f65692337e9bc2f3c866",
            nll_upper="3e2060ac8ed5c92c1d8a548d50bd768bd62e8a2d67e053f71dcd37b4276a1804",
            b_enc="d48fa164540eb531a82aaf62313bde276beb693b59ee6cdbb0043092d967f211",
            b_dec="eea0c2851481f5159ce391f66bab955af66a1c82a4fce1a8ed25dcf6c4828c73",
            samples="8e489afeca08f115b3580e811bd572266a3e5d2dadf63b02bcf64f498d3b5257",
        )),
    "rbm_bf16": (
        "lstm_pack_weights lstm_rows_gate_minor lstm_pack_weights lstm_rows_gate_minor transpose convert2d gemm_tn dropout_mask*2 lstm2_persist_fwd gemm_tn "
        "rbm_gibbs_stepped rbm_free_energy*2 weighted_sum log_loss_rows weighted_sum*2 rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn grad_rows_fanout "
        "axpby_f32*2 gemm_tn*3 lstm2_persist_bwd gemm_tn*2 lstm_unpack_grads_consume transpose gemm_tn*2 lstm_unpack_grads_consume lstm2_persist_status gemm_tn "
        "lstm2_persist_fwd gemm_tn rbm_gibbs_stepped rbm_free_energy*2 weighted_sum log_loss_rows weighted_sum*2 rbm_free_energy rbm_ais rbm_raise "
        "det_lstm_pack*2 lstm_step_det*12 dense_det lstm_step_det*12 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 dense_det "
        "det_lstm_pack*2 lstm_step_det*12 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 dense_det rbm_gibbs lstm_step_det*2 dense_det",
        dict(
            _outputs="39351ab6f3efcaa226ee61d14bdb5d334deded255d2467e571d64d694bc1a0d8",
            cond_probs="9f636cc85df83444493ec8f3a9a8ca49e3f12d46aa96bbc7995e4afa85439a09",
            free_energy="68810c79f30cce5871e739ce9073d670ef7ea8426e9bcdc6939b4cf585a13ab2",
            cost="e51423bc636c920fd4ddaaa6ae2c9fea63f6b2d0bef063fdc6dca7595a12c69e",
            nll_lower="3a1914c0c68e3280cbd70f0fff0d05a9f06aaaaeaf1492b488a1797c863092e1",
            nll_upper="72e5cf8411d7b2e0881313cdfc58dc4160c58dc27da4cfd0b514e118b9de4736",
            b_enc="d7ca637161e50e16129d247fd56678a1bfdc0934bf744c7e07a4d7c32d48cd19",
            b_dec="46263d02e2cac20df0210985e79855bbf2daee231da8452720634c7e5f6c222a",
            samples="4b646a6fde285182e353d9710a011404ea44d4d31b696c6e7dcd8afa8539f427",
        )),
    "multi_ragged": (
        "lstm_pack_weights*2 transpose convert2d gemm_tn lstm_seq_fwd dropout_fwd gemm_tn lstm_seq_fwd dropout_fwd gemm_tn rbm_gibbs_multi "
        "rbm_free_energy_multi*2 weighted_sum log_loss_rows weighted_sum*2 rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn rbm_cd_rows transpose*2 gemm_tn "
        "transpose*2 gemm_tn rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn transpose bias_grad*6 transpose gemm_tn*3 dropout_bwd lstm_seq_bwd gemm_tn "
        "dropout_bwd lstm_seq_bwd transpose gemm_tn*2 lstm_unpack_grads_consume transpose gemm_tn*2 lstm_unpack_grads_consume gemm_tn lstm_seq_fwd gemm_tn "
        "lstm_seq_fwd gemm_tn rbm_gibbs_multi rbm_free_energy_multi*2 weighted_sum log_loss_rows weighted_sum*2 rbm_free_energy rbm_ais rbm_raise "
        "rbm_free_energy rbm_ais rbm_raise rbm_free_energy rbm_ais rbm_raise det_lstm_pack*2 lstm_step_det*12 dense_det lstm_step_det*12 dense_det "
        "rbm_gibbs_multi lstm_step_det*2 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det det_lstm_pack*2 lstm_step_det*12 dense_det rbm_gibbs_multi "
        "lstm_step_det*2 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det",
        dict(
            _outputs="0882e4f2afb6e3d8f1904eb5c704de31e8ad75b9d6237bd60875a6df6df76bff",
            cond_probs="c284353d39584a6967fe2ac206e6b4f66bc6b894370db6fd9f7f39886c6ddf93",
            free_energy="b157edcf5bac347b759ea350d9e8c7fc25bc35c8d4c958771c661b6f4a227ad3",
            cost="c404565bbceb8ea80b52a8299f7f62b075f6344b3b277272845baa3cb72320b7",
            nll_lower="70765bc13525883bb8e886d15e3731a240d60695a2f585363571e06855e64775",
            nll_upper="226cae64ffe9079c555b3b60cbac260df8bba6b6bf5070212398941378480256",
            b_enc="aeeafa1c68bb6cb80c37b4d02f1afd2abe023b234dbb869b6cfe937a7a98d399",
            b_dec="42552ae0c4dc23a6e5bfc15c9af03a649321cdb2425d97f221ca011c9a7fe16a",
            samples="500151b041c547cbf23ab4f914901ab100a84303cdbeca023b79538dd767dc30",
        )),
    "multi_internal_mode": (
        "lstm_pack_weights*2 transpose convert2d gemm_tn lstm_seq_fwd dropout_fwd gemm_tn lstm_seq_fwd dropout_fwd gemm_tn rbm_gibbs_multi "
        "rbm_free_energy_multi*2 weighted_sum log_loss_rows weighted_sum*2 rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn rbm_cd_rows transpose*2 gemm_tn "
        "transpose*2 gemm_tn rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn bias_grad*6 gemm_tn lstm_seq_fwd gemm_tn lstm_seq_fwd gemm_tn rbm_gibbs_multi "
        "rbm_free_energy_multi*2 weighted_sum log_loss_rows weighted_sum*2 rbm_free_energy rbm_ais rbm_raise rbm_free_energy rbm_ais rbm_raise rbm_free_energy "
        "rbm_ais rbm_raise det_lstm_pack*2 lstm_step_det*12 dense_det lstm_step_det*12 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det rbm_gibbs_multi "
        "lstm_step_det*2 dense_det det_lstm_pack*2 lstm_step_det*12 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det rbm_gibbs_multi lstm_step_det*2 "
        "dense_det rbm_gibbs_multi lstm_step_det*2 dense_det",
        dict(
            _outputs="f121ec1d6f765fc09428635b5f4575ee042320c31210a965b3841e917b5cc987",
            cond_probs="81e396325b2cee3603c4ee3cd2b22475e80726c247070df25772dc871121e7c8",
            free_energy="323a4c7b1943fec92b62f623ab0379a4b2d424bc91e6486c9619ae31ecce8be7",
            cost="dd4d553dba9f0508b3c7f331d2829b9d76ffb60e723a5d5329ddc9071eec6760",
            nll_lower="45b6e452b07590055a1dd3b9c67f0b3b29d52e1b8a23b406a98d5840acaeffdf",
            nll_upper="bfb24c5356c60a5ee1a25776deef6d88341e722dc351114f48fbbe82fe32441f",
            b_enc="aeeafa1c68bb6cb80c37b4d02f1afd2abe023b234dbb869b6cfe937a7a98d399",
            b_dec="42552ae0c4dc23a6e5bfc15c9af03a649321cdb2425d97f221ca011c9a7fe16a",
            samples="500151b041c547cbf23ab4f914901ab100a84303cdbeca023b79538dd767dc30",
        )),
    "multi_bf16": (
        "lstm_pack_weights lstm_rows_gate_minor lstm_pack_weights lstm_rows_gate_minor transpose convert2d gemm_tn dropout_mask*2 lstm2_persist_fwd gemm_tn "
        "rbm_gibbs_multi rbm_free_energy_multi*2 weighted_sum log_loss_rows weighted_sum*2 rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn rbm_cd_rows "
        "transpose*2 gemm_tn transpose*2 gemm_tn rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn grad_rows_fanout axpby_f32*6 gemm_tn*3 lstm2_persist_bwd "
        "gemm_tn*2 lstm_unpack_grads_consume transpose gemm_tn*2 lstm_unpack_grads_consume lstm2_persist_status gemm_tn lstm2_persist_fwd gemm_tn "
        "rbm_gibbs_multi rbm_free_energy_multi*2 weighted_sum log_loss_rows weighted_sum*2 rbm_free_energy rbm_ais rbm_raise rbm_free_energy rbm_ais rbm_raise "
        "rbm_free_energy rbm_ais rbm_raise det_lstm_pack*2 lstm_step_det*12 dense_det lstm_step_det*12 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det "
        "rbm_gibbs_multi lstm_step_det*2 dense_det det_lstm_pack*2 lstm_step_det*12 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det rbm_gibbs_multi "
        "lstm_step_det*2 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det",
        dict(
            _outputs="9c53a81e4c9295b4ae1c6bb53dcd70fc58e3b4df055e441b5e018aa962d7b771",
            cond_probs="b054888aa5dafe2b0a580e74fbfbd318dfbc60e3631c18df849dfff64fa579f6",
            free_energy="1d711a3ca8707901d12aaa0c8fa3949b4278ade447c85c1d08038262180a326d",
            cost="f9376cacf520875e3554b93640986c1406e8c3fafc1f5106433a2ab6241bb8f5",
            nll_lower="74d86c883964d2c9a1ec3b3517267210fdb20568a36d61c61aecf12b0b385db7",
            nll_upper="9ecabed7e14aa16a05555947b89b85221424bdad0e08562829d5b93760981efb",
            b_enc="86e1d9c6f317f69a496abb332eb4c60d4223085969a442e2a92e2c2aeea59619",
            b_dec="b8c5daa3dd630f4f8220420dffcd3bce2f1e67d82475a38f1c8cecd4546642c8",
            samples="4d1b505d52cb5fb480898a78380be78d732b6a55793feaf864707bda8dfa0a6c",
        )),
    "multi_one_track": (
        "lstm_pack_weights*2 transpose convert2d gemm_tn lstm_seq_fwd dropout_fwd gemm_tn lstm_seq_fwd dropout_fwd gemm_tn rbm_gibbs_multi "
        "rbm_free_energy_multi*2 weighted_sum log_loss_rows weighted_sum*2 rbm_cd_rows transpose*2 gemm_tn transpose*2 gemm_tn transpose bias_grad*2 transpose "
        "gemm_tn*3 dropout_bwd lstm_seq_bwd gemm_tn dropout_bwd lstm_seq_bwd transpose gemm_tn*2 lstm_unpack_grads_consume transpose gemm_tn*2 "
        "lstm_unpack_grads_consume gemm_tn lstm_seq_fwd gemm_tn lstm_seq_fwd gemm_tn rbm_gibbs_multi rbm_free_energy_multi*2 weighted_sum log_loss_rows "
        "weighted_sum*2 rbm_free_energy rbm_ais rbm_raise det_lstm_pack*2 lstm_step_det*12 dense_det lstm_step_det*12 dense_det rbm_gibbs_multi lstm_step_det*2 "
        "dense_det rbm_gibbs_multi lstm_step_det*2 dense_det det_lstm_pack*2 lstm_step_det*12 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det "
        "rbm_gibbs_multi lstm_step_det*2 dense_det rbm_gibbs_multi lstm_step_det*2 dense_det",
        dict(
            _outputs="ffdc5f26b6c6b2da97ed51466a7c308fecbeb1913dfb76ed46fe9f1f5d920978",
            cond_probs="554f5477606b3190a2ca7a681a6f3c2710614ffc6617a46122e79f8335104c91",
            free_energy="dbd47d04d4d987bfb92604fdbfe1a87b93d622b2373b4503aadaa995755706f2",
            cost="2e8335a1b6562293ef70ad776334d5a581a6015a3b13d2aa56e27a223598192a",
            nll_lower="7e8b4383f4e179d39b777b3e0ead26682b8f93e5fb07fdff42d9ae898f7a104e",
            nll_upper="324a0cb5dfc638451c7d794b1aa23080c6892ade3306f67eb08ac1fffba75631",
            b_enc="1cea84da058586e844f9c8d6525b0189231617ed875b9276e51b1dfabab3cad5",
            b_dec="c133f755a82d9509d67250e35253cedb1a8407126575f150535feb7a4a9bab15",
            samples="5fd4fcbbeaaad02832afaa957d22afcd5d30f8285a6127e5b44f1129595428fb",
        )),
}


def expand(calls):
    """The call-list literal as a list of C entry names."""
    out = []
    for tok in calls.split():
        name, _, n = tok.partition("*")
        out += ["mnn_" + name] * int(n or 1)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_step_calls_and_bits_are_the_recorded_ones(case, monkeypatch):
    calls, out = run_case(case, monkeypatch)
    want_calls, want = PINS[case]
    assert calls == expand(want_calls)
    assert out == want


def test_one_track_multirbm_is_rnn_rbm():
    """RnnMultiRBM(tracks=["all"]) on RnnRBM's variables: the same chain ends, conditionals, free energies and costs bit for bit (the
    grouped launch equals the single one per job: test_gpu_multirbm.py; the free-energy kernel is the same kernel), and every gradient
    within 1e-4 of its largest element (the fp32 gradient bound of test_multirbm_small_shapes_fp32)."""
    one, x, y, lengths = make("rbm_ragged")
    multi = make("multi_one_track")[0]
    with torch.no_grad():
        for n in one.store.names():
            multi.store[n.replace("rbm/", "rbm_0/")].copy_(one.store[n])
    multi._packed_step = -1
    assert multi.seed == one.seed
    one.build(x, y, lengths, True, "train")
    multi.build(x, y, lengths, True, "train")
    for n in ("_outputs", "cond_probs", "free_energy", "cost", "reconstruction_cost"):
        a, b = getattr(one, n), getattr(multi, n)
        assert len(b) == 1 and a.numel() > 0 and torch.equal(a, b[0]), n
    one.backward()
    multi.backward()
    for n in one.store.names():
        a, b = one.store.gviews[n], multi.store.gviews[n.replace("rbm/", "rbm_0/")]
        assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max()), n
        assert float(a.abs().max()) > 0, n
