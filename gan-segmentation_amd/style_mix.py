"""Style-mixing plan of the generated dataset: which samples mix two latents, and at which layer.

The plan is a pure function of ``(seed, global sample index)``, so a sample is mixed the same way whatever batch, rank or GPU
count produces it (like its latents, ``Generator.draw_indexed``).  For global index ``i``:

    seed_b = seed ^ 0x5354594C454D4958            (the second latent set's seed: "STYLEMIX")
    u1     = splitmix64(seed_b ^ i)
    u2     = splitmix64(u1)
    mix    = (u1 >> 11) * 2**-53 < prob
    cutoff = 1 + u2 % (L - 1)                     (in [1, L-1]; L = 2*(max_res_log2-1) style layers)

A mixed sample takes ``w_a = mapping(z)`` for the layers ``l < cutoff`` and ``w_b = mapping(z_b)`` for the rest, where ``z_b`` is the
latent ``gsa_fill_inputs`` draws for ``(seed_b, i)``; its noise stays its own.  An unmixed sample takes ``w_a`` for every layer.
All arithmetic is on unsigned 64-bit integers (numpy uint64 wraps modulo 2**64).
"""
import numpy as np

MIX_SEED_XOR = 0x5354594C454D4958
_M64 = (1 << 64) - 1


def mix_seed(seed):
    """The seed of the second latent set."""
    return (int(seed) & _M64) ^ MIX_SEED_XOR


def splitmix64(x):
    """SplitMix64 finaliser of a uint64 array (elementwise)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def uniform_draws(seed, seed_xor, first_index, n, k):
    """float64 (n, k): per global sample ``i = first_index .. first_index+n-1`` the uniforms ``r_j = (u_j >> 11) * 2**-53`` in [0, 1)
    of the chain ``u_0 = splitmix64((seed ^ seed_xor) ^ i)``, ``u_j = splitmix64(u_{j-1})`` -- the draws of the augmentation plans."""
    idx = np.arange(n, dtype=np.uint64) + np.uint64(int(first_index) & _M64)
    u = splitmix64(np.uint64((int(seed) & _M64) ^ seed_xor) ^ idx)
    out = np.empty((n, k), np.float64)
    for j in range(k):
        if j:
            u = splitmix64(u)
        out[:, j] = (u >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return out


def mix_plan(seed, first_index, n, prob, num_layers):
    """(mix bool[n], cutoff int32[n]) of the global samples ``first_index .. first_index+n-1`` (module docstring)."""
    if num_layers < 2:
        raise ValueError("style mixing needs at least 2 layers")
    idx = np.arange(n, dtype=np.uint64) + np.uint64(int(first_index) & _M64)
    u1 = splitmix64(np.uint64(mix_seed(seed)) ^ idx)
    u2 = splitmix64(u1)
    mix = (u1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 < float(prob)
    cutoff = (np.uint64(1) + u2 % np.uint64(num_layers - 1)).astype(np.int32)
    return mix, cutoff


def layer_select(mix, cutoff, num_layers):
    """bool (n, num_layers): True where layer l of the sample takes the second latent (mixed and l >= cutoff)."""
    mix, cutoff = np.asarray(mix, dtype=bool), np.asarray(cutoff)
    return mix[:, None] & (np.arange(num_layers)[None, :] >= cutoff[:, None])
