"""8-bit Adam off the GPU (training/optimizers.py): the codec's round trip, the update against adam_update on exact
operands, and a checkpoint written and restored by the CPU runner."""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O


@pytest.mark.parametrize("kind", ["m", "v"])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1023])
def test_decode_then_encode_reproduces_codes_and_scales(kind, n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 4, n))).astype(np.float32)
    x = np.abs(x) if kind == "v" else x
    x[n // 2] = 0.0
    codes, absmax = O.q8_encode(x, kind)
    y = O.q8_decode(codes, absmax, kind)
    for k in range(O.q8_blocks(n)):  # the element that attains the maximum decodes to itself
        blk = slice(256 * k, min(256 * k + 256, n))
        assert np.abs(x[blk]).max() == absmax[k] == np.abs(y[blk]).max()
    assert not (kind == "v" and ((x > 0) & (codes == 0)).any())
    codes2, absmax2 = O.q8_encode(y, kind)
    assert np.array_equal(codes2, codes) and np.array_equal(absmax2, absmax)


@pytest.mark.parametrize("kind", ["m", "v"])
def test_a_block_decaying_under_a_zero_gradient_stays_finite_and_ends_as_the_zero_block(kind):
    """Its maximum shrinks by beta1 per step, past T / FLT_MAX where T / max is inf and 0 * inf would be NaN."""
    x = np.zeros(300, np.float32)
    x[[5, 7, 290]] = 1e-3, 2.5e-4, 1.0  # block 0 holds zeros beside the decaying values; block 1 is ordinary
    for _ in range(1000):
        x[:256] *= np.float32(0.9)
        codes, absmax = O.q8_encode(x, kind)
        x = O.q8_decode(codes, absmax, kind)
        assert np.isfinite(x).all() and x[290] == 1.0 and x[0] == 0.0
        assert absmax[0] >= O.Q8_TINY or not (absmax[0] or codes[:256].any())
    assert absmax[0] == 0.0


@pytest.mark.parametrize("argv,word", [(["--model=resnet18"], "resnet18"), (["--sync_replicas=False"], "parameter server"),
                                       (["--replicas_to_aggregate=1"], "backup workers"),
                                       (["--dp_schedule=sfb+zero"], "dp_schedule")])
def test_unsupported_combinations_are_flag_errors(argv, word):
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog", "--optimizer=adam8"] + argv)
        with pytest.raises(ValueError, match="--optimizer=adam8 .*" + word):
            dist_main.check_adam8_flags(2)
    finally:
        F.FLAGS.reset()


def test_update_agrees_with_adam_update_on_the_decoded_state():
    """beta1 = 0.5, beta2 = 0.75, small dyadic operands, every block's maximum a power of two: m', v', inv and the
    normalised values are exact in fp32 and codes of their format, so the encoded state decodes to adam_update's."""
    n = 300
    i = np.arange(n)
    m0 = np.where(i % 7 == 0, 1.0, (i % 5 - 2) * 0.25).astype(np.float32)  # in [-0.5, 1]
    v0 = np.where(i % 7 == 0, 1.0, (i % 3) * 0.25).astype(np.float32)
    g = np.where(i % 7 == 0, 1.0, (i % 2) * 0.5).astype(np.float32)      # g = 1 where m = v = 1: the maxima stay 1
    (m8, am), (v8, av) = O.q8_encode(m0, "m"), O.q8_encode(v0, "v")
    m, v = O.q8_decode(m8, am, "m"), O.q8_decode(v8, av, "v")
    assert np.array_equal(m, m0) and np.array_equal(v, v0)
    p = torch.linspace(-1, 1, n)
    args = (p, torch.from_numpy(m), torch.from_numpy(v), torch.from_numpy(g), 3, 0.125, 0.5, 0.75, 2.0 ** -10)
    p_ref, m_ref, v_ref = O.adam_update(*args)
    p2, (m8, am), (v8, av) = O.adam8_update(*args)
    assert torch.equal(p2, p_ref) and np.array_equal(am, [1.0, 1.0]) and np.array_equal(av, [1.0, 1.0])
    assert np.array_equal(O.q8_decode(m8, am, "m"), m_ref.numpy()) and np.array_equal(O.q8_decode(v8, av, "v"), v_ref.numpy())


def test_cpu_runner_checkpoint_resumes_bit_identically(tmp_path):
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner
    from tensorflow_distributed_amd.training import checkpoint

    cfg = O.Adam8bitOptimizer(0.001)
    init = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(4).items()})
    g = torch.Generator().manual_seed(2)
    b = [(torch.rand(4, 784, generator=g), torch.randint(0, 10, (4,), generator=g)) for _ in range(3)]

    def make():
        r = TorchMnistRunner(4, cfg, keep_prob=1.0)
        r.load_flat(init, {}, 0)
        return r

    a = make()
    for xy in b[:2]:
        a.train_step(*xy)
    saver = checkpoint.Saver()
    sd = saver.restore(saver.save(str(tmp_path), a.state_dict_tf(), global_step=2))
    assert all(tf_name + s in sd for _, tf_name, _ in M.PARAM_SPECS for s in ("/Adam", "/Adam_1"))
    r = make()
    r.load_state_dict_tf(sd)
    for run in (a, r):
        run.train_step(*b[2])
    n = M.NUM_PARAMS  # the padding behind the variables is in no checkpoint
    assert torch.equal(r.params()[:n], a.params()[:n]) and not torch.equal(a.params(), init)
    for x, y in zip(sum(a.applier.q8_state(), ()), sum(r.applier.q8_state(), ())):
        assert np.array_equal(x, y) and x.any()
