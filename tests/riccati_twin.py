"""TEST INFRASTRUCTURE ONLY -- I2cLinearizeOracle with a temperature PER CELL (tests/test_riccati.py).

The reference's cells each hold their own `sig_xi` (I2cCell.sig_xi; update_xi, i2c.py:976-981, writes the graph's into every cell
of the list when alpha changes): a cell appended by the MPC shift, or one whose attribute was set by hand, keeps another
temperature than the graph's. The engine's counterpart is `alpha_cell` ([T][B], enable_per_cell_alpha()); the oracle has the graph's
alpha alone. The twin re-classes an oracle INSTANCE so that cell t reads alpha_cell[:, t]; nothing of the algebra is restated:
`_forward_cell` says which cell is being computed and calls the parent, and `riccati_sweep` is inherited unchanged -- it reads what the
forward pass stored (lambda_z1_f, nu_z1_f, nu_z2_f), as the reference's does (i2c.py:278-294, 312-317, 612-678).
tests/golden/lin_pendulum_riccati_T12_cellalpha.npz pins it to the reference itself."""
import numpy as np

from oracle.i2c_linearize_numpy import I2cLinearizeOracle


class CellAlphaOracle(I2cLinearizeOracle):
    """alpha_cell: (B, T), the temperature of every cell's sig_xi; the terminal cost takes the last cell's (the cell the
    reference's end of chain reads its sig_xi_terminal from, i2c.py:475-491)."""

    _cell = 0

    @property
    def sig_xi(self):
        return self.alpha_cell[:, self._cell][:, None, None] * self.sig_xi0

    @property
    def sig_xi_terminal(self):
        if self.sig_xi_terminal_base is None:
            return None
        return self.alpha_cell[:, -1][:, None, None] * self.sig_xi_terminal_base

    def _forward_cell(self, t, mu_x, sig_x):
        self._cell = t
        return super()._forward_cell(t, mu_x, sig_x)


def with_cell_alpha(oracle, alpha_cell):
    """Re-class `oracle` (an I2cLinearizeOracle) in place; alpha_cell (B, T) or (T,)."""
    assert type(oracle) is I2cLinearizeOracle
    oracle.alpha_cell = np.broadcast_to(np.asarray(alpha_cell, float), (oracle.B, oracle.H)).copy()
    oracle.__class__ = CellAlphaOracle
    return oracle
