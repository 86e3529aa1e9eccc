"""RecurrentDiagonalGaussian (rllab/distributions/recurrent_diagonal_gaussian.py): the diagonal Gaussian itself -- its
formulas act on the last (action) axis whatever the leading axes are."""
from rllab_amd.distributions.diagonal_gaussian import DiagonalGaussian

RecurrentDiagonalGaussian = DiagonalGaussian
