from .DFSPH import DFSPHSolver
from .WCSPH import WCSPHSolver
from .PCISPH import PCISPHSolver
from .IISPH import IISPHSolver
from .PBF import PBFSolver
