"""The dropout mask stream (csrc/dropout.h) on the host, without a GPU: `lmrl_dropout_host_mask` against a Python restatement of the
documented rule built on `jax_prng.threefry2x32` (fold_in) and `jax_prng.random_bits` (the words of jax.random.bits)."""
import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
from lmrl_gym_amd import _lib, jax_prng
from lmrl_gym_amd.train import ops


def reference_mask(key, site, n, p):
    """keep[i] = bitcast((bits[i] >> 9) | 0x3F800000) - 1.0f < 1 - p in fp32, bits = jax.random.bits(fold_in(key, site), (n,))"""
    k_site = jax_prng.threefry2x32(key, (0, site))
    bits = np.asarray(jax_prng.random_bits(k_site, n), dtype=np.uint32)
    u = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return (u < np.float32(1.0) - np.float32(p)).astype(np.uint8)


KEY = jax_prng.split(jax_prng.prng_key(20240607))[1]


@pytest.mark.parametrize("site", [0, 1, 5])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 1001, 4096])
@pytest.mark.parametrize("p", [0.05, 0.25, 0.5])
def test_host_mask_equals_the_python_restatement(site, n, p):
    got = ops.dropout_host_mask(KEY, site, n, p)
    np.testing.assert_array_equal(got, reference_mask(KEY, site, n, p))


def test_keep_fraction_and_sites_differ():
    n, p = 20000, 0.25
    m0, m1, m5 = (ops.dropout_host_mask(KEY, s, n, p) for s in (0, 1, 5))
    for m in (m0, m1, m5):
        assert abs(m.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n)      # five sigma of a Bernoulli(0.75) mean
    assert (m0 != m1).mean() > 0.3 and (m1 != m5).mean() > 0.3 and (m0 != m5).mean() > 0.3      # independent masks differ on 2 p (1 - p) = 37.5 %
    other = ops.dropout_host_mask((KEY[0] ^ 1, KEY[1]), 0, n, p)
    assert (m0 != other).mean() > 0.3


def test_rate_zero_keeps_everything_and_the_size_limit_raises():
    assert ops.dropout_host_mask(KEY, 3, 513, 0.0).all()
    out = np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().lmrl_dropout_host_mask(KEY[0], KEY[1], 0, 1 << 32, 0.1, out.ctypes.data)
    assert rc != 0 and b"2^32" in _lib.lib().lmrl_last_error()
    with pytest.raises(_lib.LmrlError):
        _lib.check(rc, "lmrl_dropout_host_mask")


def test_as_key_accepts_both_forms():
    assert jax_prng.as_key(7) == jax_prng.prng_key(7)
    assert jax_prng.as_key((1, 2)) == (1, 2)
    assert jax_prng.as_key(np.array([3, 4], dtype=np.uint32)) == (3, 4)
