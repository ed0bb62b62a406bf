"""Oracle for BACE (the reference's bace/ package), written from its semantics over plain Python ints.  It works on
its own gate tuples and does not import octopuszk_amd:

    ("in", j)   input column j        ("const", v)   constant v
    ("add", a, b) / ("mul", a, b)     a, b: indices of earlier gates in the same list; the last gate is the result

  D = lowestPowerOfTwo(deg * N); beta_j = iFFT_N(column j); proof = iFFT_D(C(beta(omega_D^k)) for k < D);
  verify: proof(r) == C(beta(r)); result: FFT_D(proof)[k * D / N].
"""
from oracle import bn254
from oracle import coracle

R = bn254.R


def degree(gates):
    deg = []
    for g in gates:
        if g[0] == "in":
            deg.append(1)
        elif g[0] == "const":
            deg.append(0)
        elif g[0] == "add":
            deg.append(max(deg[g[1]], deg[g[2]]))
        else:
            deg.append(deg[g[1]] + deg[g[2]])
    return deg[-1]


def evaluate(gates, x):
    val = []
    for g in gates:
        if g[0] == "in":
            val.append(x[g[1]] % R)
        elif g[0] == "const":
            val.append(g[1] % R)
        elif g[0] == "add":
            val.append((val[g[1]] + val[g[2]]) % R)
        else:
            val.append(val[g[1]] * val[g[2]] % R)
    return val[-1]


def lowest_power_of_two(v):
    r = 1
    while r < v:
        r <<= 1
    return r


def _fft(a, omega):
    """out[i] = sum_j a[j] omega^(ij): the Python transform for small sizes, the C oracle for large ones."""
    n = len(a)
    if n <= 1024:
        b = list(a)
        bn254.serial_radix2_fft(b, omega)
        return b
    raw = coracle.fft_fr(b"".join(v.to_bytes(32, "little") for v in a), n, omega.to_bytes(32, "little"))
    return [int.from_bytes(raw[64 * i:64 * i + 32], "little") for i in range(n)]


def fft(a):
    return _fft(a, bn254.fr_root_of_unity(len(a)))


def ifft(a):
    n = len(a)
    out = _fft(a, pow(bn254.fr_root_of_unity(n), -1, R)) if n > 1 else list(a)
    c = pow(n, -1, R)
    return [v * c % R for v in out]


def columns(inputs, n, N):
    return [[inputs[i * n + j] % R for i in range(N)] for j in range(n)]


def prove(gates, inputs, n, N):
    deg = degree(gates)
    assert deg > 0 and N & (N - 1) == 0 and len(inputs) == n * N
    D = lowest_power_of_two(deg * N)
    lde = [fft(ifft(col) + [0] * (D - N)) for col in columns(inputs, n, N)]
    vals = [evaluate(gates, [lde[j][k] for j in range(n)]) for k in range(D)]
    return D, ifft(vals)


def horner(coeffs, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * r + c) % R
    return acc


def verify(gates, proof, inputs, n, N, r):
    D, coeffs = proof
    beta = [horner(ifft(col), r) for col in columns(inputs, n, N)]
    return horner(coeffs, r) == evaluate(gates, beta)


def result(proof, N):
    D, coeffs = proof
    ev = fft(list(coeffs))
    return [ev[k * (D // N)] for k in range(N)]


def naive(gates, inputs, n, N):
    return [evaluate(gates, inputs[i * n:(i + 1) * n]) for i in range(N)]
