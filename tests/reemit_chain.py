"""Support for the tests of the dust re-emission iterations of soc_amd.driver (test_driver_iterations.py, test_gpu_reemit.py): the
case of test_driver.write_case with `cellpackets`, and THE definition of correct -- the chain of the project's existing programs:

    step 0   the pipeline without `cellpackets`  ->  absorbed and emitted file
    step k   soc_amd.asoc with `iterations 1`, `nosolve`, absorptions kept, `cellpackets`, which reads the emitted file of step k-1
             and writes the absorbed file, then soc_amd.mabu.solve_emission on that file  ->  the emitted file of step k
"""
import os

import numpy as np

from soc_amd import driver, files, mabu
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User
from test_driver import write_case

CELLPACKETS = 784


def iteration_case(d, cloud, iterations=2, extra=""):
    """write_case in directory d (created), with `iterations N`, `cellpackets` and the lines of `extra`; also the same ini without
    `cellpackets` (soc0.ini: step 0 of the chain).  Returns (ini, ini0)."""
    os.makedirs(d, exist_ok=True)
    ini, _, _ = write_case(d, cloud)
    with open(ini) as fp:
        text = fp.read()
    assert "iterations 1\n" in text
    text = text.replace("iterations 1\n", "iterations %d\n" % iterations) + extra
    ini0 = os.path.join(d, "soc0.ini")
    with open(ini0, "w") as fp:
        fp.write(text)
    with open(ini, "w") as fp:
        fp.write(text + "cellpackets %d\n" % CELLPACKETS)
    return ini, ini0


def chain(ini, ini0, make_engine, N, CELLS, NFREQ, close=True):
    """The chain above in the current directory, every program with the engine make_engine() gives it (closed after it unless
    close=False: a fixture's engine).  Returns [(FABS_k, E_k) for k = 0..N] as the absorbed and the emitted file held them."""
    def done(e):
        if close:
            e.close()

    e = make_engine()
    driver.Pipeline(ini0, e, verbose=0).run(keep_files=True)
    done(e)
    U0 = User(ini)
    out = [(files.read_absorbed(U0.file_absorbed), np.array(files.mmap_emitted(U0.file_emitted, CELLS, NFREQ)))]
    for k in range(1, N + 1):
        U = User(ini)
        dusts = list(U.file_optical)
        kinds = [mabu.dust_kind(x) for x in dusts]
        U.file_optical = [x if kind != 'gsetdust' else mabu.simple_name(x) for x, kind in zip(dusts, kinds)]     # as the pipeline's transfer run
        U.NOABSORBED, U.NOMAP, U.NOSOLVE, U.ITERATIONS = 0, 1, 1, 1
        e = make_engine()
        rt = AbsorptionRun(U, e, verbose=0)
        rt.run()
        FABS = files.read_absorbed(U.file_absorbed)
        ABU = mabu.abundance_table(rt.ABU, U.SINGLE_ABU, CELLS, len(dusts))
        EM, _ = mabu.solve_emission(e, dusts, kinds, FABS, ABU)
        done(e)
        files.write_emitted(U.file_emitted, EM)
        out.append((FABS, EM))
    return out
