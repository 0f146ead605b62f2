"""src/.../loss/lattice_loss_calculator.py:5-15: a shell over the coordinates' calculator.  As in the reference its constructor
passes no parameters on, so it cannot be instantiated; create_loss_calculator builds the lattice loss from LOSS_BY_ALGO."""
from .coordinates_loss_calculator import CoordinatesLossCalculator


class LatticeLossCalculator(CoordinatesLossCalculator):
    def __init__(self):
        super().__init__()
