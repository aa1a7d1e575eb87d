"""Large fixture weights of the multi-scale discriminator, regenerated from a seed instead of stored: a hidden-16 MSD holds 0.46 M
floats, and trainstep_msd.npz holds a second set; random fp32 does not compress, so stored they would add 1.9 MB to each file, whose
recorded results already take 0.93 MB and 0.34 MB — past the 1 MiB that a newly committed file may weigh (fixtures of about
1 MB each).  numpy's legacy RandomState stream is frozen across numpy versions, so
`seeded(seed, shape)` is the same array wherever it runs; make_msd_golden.py writes these values INTO the reference module before it
records anything, and the fixtures store `[seed]` under "seed::<key>" where a state_dict tensor is one of them."""
import numpy as np

MIN_SEEDED = 1024      # state_dict tensors with at least this many elements are seeded, smaller ones are stored


def seeded(seed, shape):
    n = int(np.prod(shape))
    fan_in = max(1, n // shape[0])
    return (np.random.RandomState(int(seed)).standard_normal(n) / np.sqrt(fan_in)).astype(np.float32).reshape(shape)


def state_dict_from(z, prefix, shapes):
    """The state_dict stored under `prefix` in the npz `z`: stored tensors as they are, seeded ones regenerated (shapes: key -> shape)."""
    out = {}
    for k in z.files:
        if k.startswith(prefix + "sd::"):
            out[k[len(prefix) + 4:]] = np.asarray(z[k])
        elif k.startswith(prefix + "seed::"):
            key = k[len(prefix) + 6:]
            out[key] = seeded(int(z[k][0]), tuple(shapes[key]))
    return out
