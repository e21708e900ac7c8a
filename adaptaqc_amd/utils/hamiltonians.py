# (C) Copyright IBM 2025.
#
# This code is licensed under the Apache License, Version 2.0. You may
# obtain a copy of this license in the LICENSE.txt file in the root directory
# of this source tree or at http://www.apache.org/licenses/LICENSE-2.0.
#
# Any modifications or derivative works of this code must retain this
# copyright notice, and modified files need to carry a notice indicating
# that they have been altered from the originals.
#
# Modified for adaptaqc_amd: this file restates the reference file named in its docstring
# (qiskit-community/adapt-aqc) on top of the MI355X engine (libaqchip); it has been altered
# from the original.

"""Model Hamiltonians as Pauli-label dicts (reference adaptaqc/utils/hamiltonians.py).

The reference builds OpenFermion ``QubitOperator``s and converts them with
``convert_qubit_op_to_pauli_dict``; here ``heisenberg_hamiltonian`` returns the ``{label: real
coefficient}`` dict that ``expectation_value_of_pauli_operator`` takes directly (labels in qiskit
order: the rightmost character is qubit 0).  The Anderson model (hamiltonians.py:42-77) needs
OpenFermion's Jordan-Wigner transform and is not provided.
"""


def _label(n, ops):
    chars = ["I"] * n
    for q, p in ops:
        chars[n - 1 - q] = p
    return "".join(chars)


def heisenberg_hamiltonian(n=4, jx=1.0, jy=0.0, jz=0.0, hx=0.0, hy=0.0, hz=0.0, periodic_bc=False):
    """hamiltonians.py:21-39:
    H = -sum_over_nn(j_x*X_i*X_(i+1) + j_y*Y_i*Y_(i+1) + j_z*Z_i*Z_(i+1)) - sum(h_x*X_i + h_y*Y_i + h_z*Z_i).

    Terms with a zero coefficient are left out (the reference keeps them in its QubitOperator
    until OpenFermion's own simplification); coefficients of a label that occurs twice (the n = 2
    periodic chain) add."""
    n = int(n)
    ham = {}

    def add(label, coeff):
        if coeff == 0:
            return
        ham[label] = ham.get(label, 0.0) + float(coeff)

    for i in range(n if periodic_bc else n - 1):
        j = 0 if (i == n - 1 and periodic_bc) else i + 1
        for p, c in (("X", jx), ("Y", jy), ("Z", jz)):
            add(_label(n, [(i, p), (j, p)]), -c)
    for i in range(n):
        for p, c in (("X", hx), ("Y", hy), ("Z", hz)):
            add(_label(n, [(i, p)]), -c)
    return ham
