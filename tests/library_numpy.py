"""A numpy statement of the library build (soc_library.py:127-217), independent of the C restatement: shared by
tests/test_library.py, which holds the restatement to it, and tools/exp_library.py, which times it."""
import numpy as np

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def numpy_build(N, ABS3, log10=np.log10):
    """Steps (a)-(e) with numpy float32 scalars and arrays in the order the reference writes them: N + N^2 masked passes, then the
    winner of every bin by sorting (bin, distance, cell).  Where the reference leaves a case open (see library_host.c) the indices
    are clipped before they index and the distance is summed in float32.  log10: numpy's, or the restatement's libm log10f where
    the two differ in a last bit on a case's inputs (numpy brings its own vectorised logarithm)."""
    IREF = log10(np.clip(np.asarray(ABS3, f32), f32(1.0e-25), f32(1.0)))
    assert IREF.dtype == np.float32

    def axis(a, b):
        d = (b - a) / f32(N) + f32(0.1)
        a, b = a - d, b + d
        dI = np.clip(f32(1.001) * (b - a) / f32(N), f32(1.0e-30), f32(1.0e30))
        I = a + f32(0.499) * dI
        assert I.dtype == np.float32 and dI.dtype == np.float32
        return I, dI

    I0, dI0 = axis(IREF[:, 0].min(), IREF[:, 0].max())
    I1, dI1 = np.zeros(N, f32), np.zeros(N, f32)
    I2, dI2 = np.zeros((N, N), f32), np.zeros((N, N), f32)
    for i in range(N):
        in0 = np.abs(IREF[:, 0] - (I0 + f32(i) * dI0)) < f32(0.5) * dI0
        if in0.sum() < 1:
            I1[i], dI1[i] = 100.0, 0.001
        else:
            I1[i], dI1[i] = axis(IREF[in0, 1].min(), IREF[in0, 1].max())
        for j in range(N):
            both = in0 & (np.abs(IREF[:, 1] - (I1[i] + f32(j) * dI1[i])) < f32(0.5) * dI1[i])
            if both.sum() < 2:
                I2[i, j], dI2[i, j] = 100.0, 0.001
            else:
                I2[i, j], dI2[i, j] = axis(IREF[both, 2].min(), IREF[both, 2].max())
    a, b = f32(100.0), f32(0.001)
    for i in range(N):
        for j in range(N):
            if I2[i, j] < 99.0:
                a, b = I2[i, j], dI2[i, j]
            else:
                I2[i, j], dI2[i, j] = a, b
    X = (IREF[:, 0] - I0) / dI0
    I = np.clip(np.round(X).astype(np.int64), 0, N - 1)
    Y = (IREF[:, 1] - I1[I]) / dI1[I]
    J = np.clip(np.round(Y).astype(np.int64), 0, N - 1)
    Z = (IREF[:, 2] - I2[I, J]) / dI2[I, J]
    K = np.clip(np.round(Z).astype(np.int64), 0, N - 1)
    dis = (np.abs(X - I.astype(f32)) + np.abs(Y - J.astype(f32))) + np.abs(Z - K.astype(f32))
    assert dis.dtype == np.float32
    b = K + N * (J + N * I)
    order = np.lexsort((np.arange(len(b)), dis, b))                   # by bin, then distance, then cell
    first = order[np.concatenate([[True], b[order][1:] != b[order][:-1]])]
    IND = np.full(N ** 3, -1, np.int32)
    XX, YY, ZZ = np.zeros(N ** 3, f32), np.zeros(N ** 3, f32), np.zeros(N ** 3, f32)
    XX[b[first]], YY[b[first]], ZZ[b[first]] = X[first], Y[first], Z[first]
    ok = dis[first] <= f32(1.5)
    IND[b[first][ok]] = first[ok]
    shape = (N, N, N)
    return dict(N=N, I0=I0, dI0=dI0, I1=I1, dI1=dI1, I2=I2, dI2=dI2, IND=IND, X=XX.reshape(shape), Y=YY.reshape(shape), Z=ZZ.reshape(shape))


GRID = ("I0", "dI0", "I1", "dI1", "I2", "dI2")


def same_build(a, b):
    return [k for k in GRID + ("X", "Y", "Z") if not np.array_equal(bits(a[k]), bits(b[k]))] + ([] if np.array_equal(a["IND"], b["IND"]) else ["IND"])
