// chem_cells.hip -- the stiff integrators over a per-cell interval (chem_solve_cells: EDC's chemistryPtr_->solve(tauStar)),
// the DT = const double* instantiations of chem.hip's kernels, compiled apart from the scalar ones (see chem.hip)
#define DFMI_CHEM_CELLS 1
#include "chem.hip"
