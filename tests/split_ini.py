"""A small ini run of the absorption stage for the packet-splitting tests: model files, the ini text and the run."""
import os

import numpy as np

from soc_amd import files, synth
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User

FREQ = [1.0e14, 3.0e14, 6.0e14]
BG = [1e-13, 2e-13, 1.5e-13]


def dust_cross_sections():
    """(ABS, SCA) per frequency as written to the dust file below"""
    return [(2.0e-7 * f / 3.0e14, 6.0e-7) for f in FREQ]


def write_model(d, cloud, extra="", bgpackets=300):
    d = str(d)
    os.makedirs(d, exist_ok=True)
    cloud.write(os.path.join(d, "m.cloud"))
    with open(os.path.join(d, "m.dust"), "w") as fp:
        fp.write("eqdust\n 1.0e-7\n 1.0e-4\n%d\n" % len(FREQ))
        for f, (a, s) in zip(FREQ, dust_cross_sections()):
            fp.write(" %.5e  0.6  %.5e  %.5e\n" % (f, a, s))
    dsc, csc = synth.hg_scattering_table(0.6, 500)
    files.write_scattering_functions(os.path.join(d, "m.dsc"), np.tile(dsc, (len(FREQ), 1)), np.tile(csc, (len(FREQ), 1)))
    np.asarray(BG, np.float32).tofile(os.path.join(d, "bg.bin"))
    ini = ("gridlength 0.05\ncloud %s/m.cloud\noptical %s/m.dust\ndsc %s/m.dsc 500\nbackground %s/bg.bin\n"
           "bgpackets %d\nseed 0.7853981634\niterations 1\nabsorbed %s/abs.data\nnosolve\nnomap\ndevice g\nverbose 0\n"
           % (d, d, d, d, bgpackets, d))
    ini += extra
    path = os.path.join(d, "m.ini")
    with open(path, "w") as fp:
        fp.write(ini)
    return path


def run_ini(engine, d, split=1, cloud=None, extra="", bgpackets=300, seed=None):
    """Runs the ini file in directory d.  Returns dict(absorbed [CELLS, NFREQ] as written, packet_info, launches (of a
    SplitOracleEngine, else None), stats (split_stats), run, nfreq)"""
    from split_cases import model
    cloud = model("oct4b") if cloud is None else cloud
    text = ("split %d\n" % split if split is not None else "") + extra + ("seed %.10f\n" % seed if seed is not None else "")
    ini = write_model(d, cloud, text, bgpackets)
    here = os.getcwd()
    os.chdir(str(d))
    try:
        U = User(ini)
        if hasattr(engine, "split_stats"):
            engine.split_stats(reset=True)
        run = AbsorptionRun(U, engine, verbose=0)
        run.run()
        out = dict(absorbed=np.array(files.read_absorbed(os.path.join(str(d), "abs.data"))), packet_info=np.fromfile("packet.info", np.int32),
                   launches=getattr(engine, "split_launches", None), run=run, nfreq=len(FREQ),
                   stats=engine.split_stats(reset=True) if hasattr(engine, "split_stats") else None)
    finally:
        os.chdir(here)
    return out
