"""The map products of an ASOC run (reference ASOC.py:2903-3958): surface-brightness maps, flat and Healpix, and their split by
hierarchy level, optical-depth and column-density images, polarisation maps, the optical depths towards the point sources.
MapProducts is the part of soc_amd.asoc.AbsorptionRun that writes them; the kernels are the engine's (soc_amd/csrc/soc_map.hip)."""
import numpy as np

from . import files, launch
from .launch import PLANCK, PARSEC


def scale_emission_once(KK, FREQ, column):
    """The emission in the map kernels' unit as float32((KK * FREQ in float64) * EMITTED), the factor rounded ONCE: the flat maps
    (write_maps; ASOC.py:3104-3105, KK of :2997-2998) and both polarisation maps (write_polmaps, :3788; write_healpix_polmaps, :3944)"""
    return np.asarray(float(KK) * float(FREQ) * column, np.float32)


def scale_emission_twice(KK, FREQ, column):
    """The same as EMITTED * float32(KK) * float32(FREQ), TWO float32 products whose last bit can differ from scale_emission_once:
    the Healpix maps (write_healpix_maps; ASOC.py:3283) and the per-level maps (write_level_maps, :3404)"""
    return np.asarray(column * np.float32(KK) * np.float32(float(FREQ)), np.float32)


def near_mapum(FREQ, singles):
    """The `mapum` rule of the flat maps (ASOC.py:3059-3062): FREQ lies within 0.5 % of a listed frequency, compared in float64.
    The polarisation maps have a rule of their own: MapProducts.polmap_frequencies, 1 % in float32 (ASOC.py:3755-3762)."""
    return not np.min(np.abs(FREQ - singles)) / FREQ > 0.005


class MapProducts:
    """Writes every map product of a run.  What it needs from the run that inherits it:
    U, eng, cloud, rank, FFREQ, NFREQ, lib_col, WITH_ABU; log(), _optical_for(IFREQ) and emitted_range()."""

    def _view(self):
        """(views, centre, KK, LENGTH_f, pix): [(DIR, RA, DE)] per observer direction, the map centre (ASOC_aux.py:791-793), KK that
        takes emission x frequency to Jy/sr (ASOC.py:2997-2998), the kernels' LENGTH, the FITS pixel GL*MAP_DX / distance (1 kpc unless given)"""
        U, c = self.U, self.cloud
        NDIR, ODIR, RA, DE = launch.set_observer_directions(U.OBS_THETA, U.OBS_PHI)
        centre = U.MAPCENTRE if U.MAPCENTRE[0] > -1e7 else (0.5 * c.NX, 0.5 * c.NY, 0.5 * c.NZ)
        KK = (1.0e23 / launch.FACTOR) * PLANCK / (4.0 * np.pi) * (U.GL * PARSEC)
        _, LENGTH_f = launch.kernel_literals(U.GL)
        pix = U.GL * U.MAP_DX / (U.DISTANCE if U.DISTANCE > 0.0 else 1000.0)
        return [(ODIR[idir], RA[idir], DE[idir]) for idir in range(NDIR)], centre, KK, LENGTH_f, pix

    def _mapped_range(self):
        """(I1, I2) of the frequencies with emission to map: the emitted range -- with `libmaps` the whole table, whatever `remit` says (ASOC.py:202-204)"""
        I1, I2 = self.emitted_range()
        return (0, self.NFREQ - 1) if self.U.LIB_MAPS else (I1, I2)

    def _inside_wavelength(self):
        """(I1, sel): the frequencies of the mapped range inside `wavelength` -- the selection of the level maps, the Healpix maps
        and the Healpix polarisation maps; with `libmaps` those of its file only (ASOC.py:3234-3250)"""
        U = self.U
        I1, I2 = self._mapped_range()
        return I1, [i for i in range(I1, I2 + 1) if U.MAP_FREQ[0] <= float(self.FFREQ[i]) <= U.MAP_FREQ[1]
                    and not (U.LIB_MAPS and i not in self.lib_col)]

    def _flat_selection(self):
        """(I1, sel) of the flat maps: sel = [(IFREQ, save_spe, save_tau, save_colden)] in ascending frequency, what is computed
        at each frequency inside `wavelength` (ASOC.py:3032-3062)"""
        U = self.U
        I1, I2 = self._mapped_range()
        singles = np.asarray(getattr(U, "SINGLE_MAP_FREQ", []), np.float64)
        savetau = np.asarray(getattr(U, "savetau_freq", []), np.float64)
        sel = []
        first_freq = True
        for IFREQ in range(self.NFREQ):
            FREQ = float(self.FFREQ[IFREQ])
            if U.LIB_MAPS and IFREQ not in self.lib_col:           # the loop is over the whole table, the others are skipped (ASOC.py:3032-3038)
                continue
            save_spe = (IFREQ >= I1) and (IFREQ <= I2)
            if (FREQ < U.MAP_FREQ[0]) or (FREQ > U.MAP_FREQ[1]):
                continue
            save_tau, save_colden = 0, 0
            if len(savetau) > 0:                                   # ASOC.py:3048-3058
                if np.min(np.abs((savetau - FREQ) / FREQ)) < 0.001:
                    save_tau = 1
                if (save_tau == 0) and first_freq and (np.min(savetau) <= 0.0):
                    save_colden = 1                                # `savetau file -1`: column density, with the first mapped frequency
            first_freq = False
            if len(singles) > 0 and not near_mapum(FREQ, singles):
                save_spe = False
            if save_spe or save_tau or save_colden:
                sel.append((IFREQ, save_spe, save_tau, save_colden))
        return I1, sel

    def _emission(self, EMITTED, I1, KK, scale):
        """emission(IFREQ, save_spe) -> float32[CELLS]: scale (scale_emission_once or _twice) of the frequency's column of EMITTED -- with
        `libmaps` the column of the library's emission (ASOC.py:3104-3105) -- or zeros for a frequency mapped for its optical depth only"""
        def emission(IFREQ, save_spe=True):
            if not save_spe:
                return np.zeros(self.cloud.CELLS, np.float32)
            col = self.lib_col[IFREQ] if self.U.LIB_MAPS else IFREQ - I1
            return scale(KK, self.FFREQ[IFREQ], EMITTED[:, col])
        return emission

    def _open_map_file(self, name, *pairs):
        """a map file opened for writing, with its header: the int32 pairs (NPIX.x, NPIX.y first)"""
        fp = open(name, "wb")
        for pair in pairs:
            np.asarray(pair, np.int32).tofile(fp)
        return fp

    def _open_level_file(self, idir, images):
        """map_dir_XX_L.bin of `maplevels 1`: int32 NPIX.x, NPIX.y, int32 [images, LEVELS]; the caller appends per image LEVELS float32
        planes [Jy/sr], plane l what the cells of level l add to the plain map's image."""
        return self._open_map_file("map_dir_%02d_L.bin" % idir, self.U.NPIX, [images, self.cloud.LEVELS])

    def _map_levels(self):
        return getattr(self.U, "MAP_LEVELS", 0) > 0

    def _map_walks(self, sel, emission, views, centre, LENGTH_f, healpix=0):
        """The one map loop: yields what _map_blocks yields.  `maplevels 1` and `mapping nx ny dx NF` (2 <= NF <= 998) go through it, the
        first with the fourth member MAPL; otherwise every frequency of sel is a batch of one from engine.map, whose second array is
        the column density where save_colden asks for it."""
        U, e = self.U, self.eng
        if self._map_levels() or 2 <= U.FAST_MAP <= 998:
            yield from self._map_blocks(sel, emission, views, centre, LENGTH_f, healpix=healpix, levels=self._map_levels())
            return
        hp = dict(healpix=healpix) if healpix else {}
        for q in sel:
            IFREQ, save_spe, _, save_colden = q
            ABS, SCA = self._optical_for(IFREQ)
            EMIT = emission(IFREQ, save_spe)
            planes = []
            for d, ra, de in views:
                MAP, TAU = e.map(EMIT, d, ra, de, U.NPIX, U.MAP_DX, centre, ABS, SCA, INTOBS=U.INTOBS, save_colden=save_colden,
                                 LENGTH=LENGTH_f, **hp)
                planes.append(((MAP,), (TAU,), TAU))
            yield [q], planes

    def _map_blocks(self, sel, emission, views, centre, LENGTH_f, healpix=0, levels=False):
        """`mapping nx ny dx NF` (2 <= NF <= 998; ASOC.py:3442-3568): the frequencies of sel = [(IFREQ, save_spe, save_tau,
        save_colden)] in batches of at most min(NF, engine.map_block_max).  A batch is uploaded once -- emission(IFREQ, save_spe)
        as the columns of EMITX[CELLS, nf], the opacities _optical_for sets for the plain path (with abundances the per-cell
        ones it builds, read back into OPTX[CELLS, nf, 2]) -- and mapped for every view = (DIR, RA, DE).  Yields (batch,
        [(MAPX, TAUX, COLDEN) per view]); with levels (`maplevels 1`) every view's tuple has a fourth member, the planes
        MAPL[nf, LEVELS, ...] of engine.map_block_levels for the same batch and view."""
        U, e, c = self.U, self.eng, self.cloud
        nb = max(1, min(int(U.FAST_MAP), int(e.map_block_max)))
        for b0 in range(0, len(sel), nb):
            batch = sel[b0:b0 + nb]
            EMITX = np.zeros((c.CELLS, len(batch)), np.float32)
            ABSX, SCAX = np.zeros(len(batch), np.float32), np.zeros(len(batch), np.float32)
            OPTX = np.zeros((c.CELLS, len(batch), 2), np.float32) if self.WITH_ABU else None
            for k, (IFREQ, save_spe, _, _) in enumerate(batch):
                ABSX[k], SCAX[k] = self._optical_for(IFREQ)
                if OPTX is not None:
                    OPTX[:, k, :] = np.asarray(e.read_opt(), np.float32).reshape(c.CELLS, 2)
                if save_spe:
                    EMITX[:, k] = emission(IFREQ, save_spe)
            e.set_map_block(EMITX, ABSX, SCAX, OPTX)
            del EMITX, OPTX
            planes = [e.map_block(d, ra, de, U.NPIX, U.MAP_DX, centre, INTOBS=U.INTOBS, LENGTH=LENGTH_f, healpix=healpix)
                      for d, ra, de in views]
            if levels:
                planes = [tuple(p) + (e.map_block_levels(d, ra, de, U.NPIX, U.MAP_DX, centre, INTOBS=U.INTOBS, healpix=healpix),)
                          for p, (d, ra, de) in zip(planes, views)]
            yield batch, planes
        e.set_map_block(None)

    def write_maps(self, EMITTED):
        """Surface-brightness maps from the emission (ASOC.py:2924-3177, the plain `Mapping` path): for every
        direction map_dir_XX.bin = int32 NPIX.x, NPIX.y + one float32 [NPIX.y, NPIX.x] image [Jy/sr] per selected
        frequency.  `perspective` gives the longitude x latitude image seen from that position.  Optical-depth
        images for `savetau` frequencies are written as <file>_tau_<um>.bin, the column density (`savetau file -1`) as
        <file>_colden.fits; `fits` with `mapum` gives one FITS image per direction and frequency instead.  NPIX.y < 0:
        write_healpix_maps.  Polarisation maps: write_polmaps.
        `maplevels 1` (not a key of the reference) adds map_dir_XX_L.bin per direction (map_dir_00_L.bin for a Healpix map):
        int32 NPIX.x, NPIX.y, int32 [images, LEVELS], then for every image of the plain file, in its order, LEVELS float32 planes
        [Jy/sr] -- plane l is the plain map with the emission of all cells not on hierarchy level l set to zero, so the planes of
        an image add up to it.  The frequencies then go through _map_blocks in batches of min(max(1, FAST_MAP), map_block_max);
        the plain products are the same bytes.  With `fits` + `mapum` the level file is still this .bin.  maplevels has no
        effect on the `polmap` products (write_polmaps, write_healpix_polmaps)."""
        U = self.U
        if U.NPIX[1] == 0:
            self.log("mapping with NPIX.y == 0: neither the flat (NPIX.y > 0, ASOC.py:2924) nor the Healpix branch (NPIX.y < 0, :3185)")
            return
        if U.FAST_MAP >= 999:
            return self.write_level_maps(EMITTED)
        if U.NPIX[1] < 0:
            return self.write_healpix_maps(EMITTED)
        I1, sel = self._flat_selection()
        views, centre, KK, LENGTH_f, pix = self._view()
        NDIR = len(views)
        # `fits` together with `mapum`: one FITS file per direction and selected frequency instead of map_dir_XX.bin
        # (ASOC.py:2977-2996); the header is MakeFits' (files.write_fits)
        using_fits = (getattr(U, "FITS", 0) > 0) and (len(getattr(U, "SINGLE_MAP_FREQ", [])) > 0)
        fps = [self._open_map_file("map_dir_%02d.bin" % idir, U.NPIX) for idir in range(NDIR)] if self.rank == 0 and not using_fits else []
        # (the level files are .bin also where `fits` + `mapum` turn the plain maps into FITS files)
        lfps = [self._open_level_file(idir, sum(1 for q in sel if q[1])) for idir in range(NDIR)] if self.rank == 0 and self._map_levels() else []

        def write(IFREQ, idir, MAP, TAU, save_spe, save_tau, save_colden):
            """the files of one frequency and direction; TAU: the optical depth, or with save_colden the column density"""
            um = launch.C_LIGHT / float(self.FFREQ[IFREQ]) * 1.0e4
            ums = '%.0f' % um if um > 20.0 else ('%.1f' % um if um > 2.0 else '%.2f' % um)
            suffix = '_dir%d' % idir if NDIR > 1 else ''
            tail = '' if NDIR == 1 else '_%03d' % idir
            if save_spe:
                if using_fits:                                  # :3143-3148
                    files.write_fits("%s_%s%s.fits" % (U.FITS_PREFIX, ums, tail), MAP, U.FITS_RA, U.FITS_DE, pix)
                else:
                    np.asarray(MAP, np.float32).tofile(fps[idir])
            if save_colden:                                     # always a FITS image in the reference (:3152-3159)
                files.write_fits('%s_colden%s%s.fits' % (U.file_savetau, suffix, tail), TAU, U.FITS_RA, U.FITS_DE, pix)
            if save_tau:                                        # :3160-3171
                name = '%s_tau_%s%s%s' % (U.file_savetau, ums, suffix, tail)
                if using_fits:
                    files.write_fits(name + '.fits', TAU, U.FITS_RA, U.FITS_DE, pix)
                else:
                    np.asarray(TAU, np.float32).tofile(name + '.bin')

        for batch, planes in self._map_walks(sel, self._emission(EMITTED, I1, KK, scale_emission_once), views, centre, LENGTH_f):
            if self.rank != 0:
                continue
            for idir, p in enumerate(planes):
                MAPX, TAUX, COLDEN = p[:3]
                for k, (IFREQ, save_spe, save_tau, save_colden) in enumerate(batch):
                    write(IFREQ, idir, MAPX[k], COLDEN if save_colden else TAUX[k], save_spe, save_tau, save_colden)
                    if save_spe and lfps:
                        np.asarray(p[3][k], np.float32).tofile(lfps[idir])
        for fp in fps + lfps:
            fp.close()

    def write_healpix_maps(self, EMITTED):
        """`mapping NSIDE -1 dx`: all-sky map of the emission seen from `perspective` (HealpixMapping, kernel_ASOC_map.c),
        file layout of ASOC.py:3185-3320: map_dir_00_H.bin = int32 [NPIX.x, NPIX.y], int32 [frequencies, LEVELS], then one
        float32 [12*NSIDE^2] map [Jy/sr] per frequency of the emitted range inside `wavelength`.
        The reference itself stops in this branch with a NameError (SAVE_COLDEN is never assigned, :3291/:3297) after
        writing the two headers; this writes the file its loop describes, with SAVE_COLDEN = 0 (no column-density file:
        its savetau tests compare a list with a float, :3303-3306)."""
        U = self.U
        NSIDE = int(U.NPIX[0])
        I1, sel = self._inside_wavelength()
        views, centre, KK, LENGTH_f, _ = self._view()
        fp = lfp = None
        if self.rank == 0:
            fp = self._open_map_file("map_dir_%02d_H.bin" % 0, U.NPIX, [len(sel), self.cloud.LEVELS])     # NDIR = 1 for Healpix maps (ASOC.py:2917)
            lfp = self._open_level_file(0, len(sel)) if self._map_levels() else None
        for batch, planes in self._map_walks([(i, True, 0, 0) for i in sel], self._emission(EMITTED, I1, KK, scale_emission_twice),
                                             views[:1], centre, LENGTH_f, healpix=NSIDE):
            for k in range(len(batch)):
                if fp:
                    np.asarray(planes[0][0][k], np.float32).tofile(fp)
                if lfp:
                    np.asarray(planes[0][3][k], np.float32).tofile(lfp)
        for f in filter(None, (fp, lfp)):
            f.close()

    def write_level_maps(self, EMITTED):
        """`mapping nx ny dx 999` (a fourth argument >= 999): one image per hierarchy level (ASOC.py:3323-3438 -> the Mapping of
        kernel_ASOC_map_H.c).  For every direction map_dir_XX_H.bin = int32 NPIX.x, NPIX.y, then int32 number of frequencies
        written, LEVELS, then per frequency of the emitted range inside `wavelength` LEVELS float32 images [NPIX.y, NPIX.x]
        [Jy/sr]: image l holds the emission of the cells of level l, attenuated by everything in front of them.  `perspective`
        gives the longitude x latitude images seen from that position.  `mapum` selects nothing here (ASOC.py:3363-3375), and
        `mapint`, `threshold` and `roimap` have no effect: that kernel tests none of them.  With abundances the extinction is
        the per-cell sum (`singleabu`, `optishalf` included), which the reference has under a macro it never defines.
        The walk is that kernel file's own, bit for bit: on a hierarchy it loses a ray where the ray climbs out of an octet into
        a root leaf, so the images hold only what lies in front of that point."""
        U, e = self.U, self.eng
        I1, sel = self._inside_wavelength()
        views, centre, KK, _, _ = self._view()
        emission = self._emission(EMITTED, I1, KK, scale_emission_twice)
        names = ["map_dir_%02d_H.bin" % idir for idir in range(len(views))]
        fps = [self._open_map_file(name, U.NPIX, [len(sel), self.cloud.LEVELS]) for name in names] if self.rank == 0 else []
        for IFREQ in sel:
            ABS, SCA = self._optical_for(IFREQ)
            EMIT = emission(IFREQ)
            for idir, (d, ra, de) in enumerate(views):
                MAP = e.map_levels(EMIT, d, ra, de, U.NPIX, U.MAP_DX, centre, ABS, SCA, INTOBS=U.INTOBS)
                if self.rank == 0:
                    np.asarray(MAP, np.float32).tofile(fps[idir])
        for fp in fps:
            fp.close()
        return names

    def polarisation_field(self, healpix=False, R=None):
        """The three B files of `polmap` (the layout of the cloud file: every cell, parents included) with the polarisation
        reduction factor R of `polred` encoded in the length of the vectors, B * R / sqrt(B^2 + 1e-10) (ASOC.py:3676-3720):
        `adhoc` -- R from the dust temperatures of the `temperature` file; `rhofun_<threshold>_<width>` -- from the density
        (times `density`); anything else -- a plain file [cells, {R}], clipped to [1e-6, 0.999999].  polstat 3 uses the
        vectors as they are.  healpix: the encoding of the Healpix branch (ASOC.py:3836-3872), B * R / sqrt(B^2) with a
        file's R as it is.  R: the factors R[cells] themselves where the ini names no `polred` -- treated as a plain file's are."""
        U, c = self.U, self.cloud
        BB = [np.asarray(files.read_temperature(f, c), np.float32) for f in U.BFILES[:3]]
        polred = getattr(U, "file_polred", "")
        given = None
        if len(polred) == 0 and R is not None:
            polred, given = "the polarisation reduction factors of the emission stage", np.asarray(R, np.float32)
        if U.POLSTAT != 3 and len(polred) > 0:
            if polred == 'adhoc':
                R = files.read_temperature(U.file_temperature, c)
                R = (R - 13.3) / 2.0 + 1.0e-4
                R = np.exp(R) / (np.exp(R) + np.exp(-R))
            elif polred.find('rhofun') >= 0:
                s = polred.split('_')
                th, sw = float(s[1]), float(s[2])
                R = files.read_temperature(U.file_cloud, c)             # the density as the file holds it (read_otfile)
                if U.KDENSITY != 1.0:
                    R *= U.KDENSITY
                R = np.clip(R, 0.1, 1e10)
                R = 0.5 * (1.0 + np.tanh((np.log10(th) - np.log10(R)) / sw))
            else:
                R = np.fromfile(polred, np.float32)[1:] if given is None else given
                if not healpix:
                    R = np.clip(R, 1.0e-6, 0.999999)
                if R.size != c.CELLS:
                    raise files.FileError("%s: %d polarisation reduction factors for %d cells" % (polred, R.size, c.CELLS))
            if healpix:
                R = R / np.sqrt(BB[0] ** 2 + BB[1] ** 2 + BB[2] ** 2)
            else:
                R = R / np.sqrt(BB[0] ** 2 + BB[1] ** 2 + BB[2] ** 2 + 1.0e-10)
            for k in range(3):
                BB[k] *= R
        return [np.ascontiguousarray(b, np.float32) for b in BB]

    def polmap_frequencies(self):
        """(I1, sel): the frequencies that get a polarisation map (ASOC.py:3755-3762): those of the emitted range within 1 % of a
        `mapum` wavelength, compared in float32 -- or, without `mapum`, inside `wavelength`.  (The flat maps: near_mapum.)"""
        U, FFREQ = self.U, self.FFREQ
        I1, I2 = self.emitted_range()
        singles = np.asarray(getattr(U, "SINGLE_MAP_FREQ", []), np.float32)
        if len(singles) > 0:
            return I1, [i for i in range(I1, I2 + 1) if not np.min(np.abs(FFREQ[i] - singles)) > 0.01 * FFREQ[i]]
        return I1, [i for i in range(I1, I2 + 1) if not ((FFREQ[i] < U.MAP_FREQ[0]) or (FFREQ[i] > U.MAP_FREQ[1]))]

    def _polmap_steps(self, EMITTED, R, I1, sel, KK, healpix):
        """The frequency loop of both polarisation-map writers; yields (IFREQ, EMIT, ABS, SCA).  The field is set once -- or, with
        R[CELLS, columns of EMITTED] from the emission stage, at every frequency with its column -- and freed at the end."""
        e = self.eng
        emission = self._emission(EMITTED, I1, KK, scale_emission_once)
        if R is None:
            e.set_bfield(*self.polarisation_field(healpix=healpix))
        for IFREQ in sel:
            ABS, SCA = self._optical_for(IFREQ)
            if R is not None:
                e.set_bfield(*self.polarisation_field(healpix=healpix, R=R[:, IFREQ - I1]))
            yield IFREQ, emission(IFREQ), ABS, SCA
        e.set_bfield(None)

    def write_polmaps(self, EMITTED, R=None):
        """`polmap bx by bz`: polarisation maps from the emission (ASOC.py:3651-3801 -> PolMapping): for every selected
        frequency and observer direction polmap_<um>_<dir>.fits with data [4, NPIX.y, NPIX.x] -- I, Q, U [Jy/sr] and the
        column density (polstat 0), the line-of-sight statistics rT, rI, jT, jI of the field (polstat 1), or <B>, <B_LOS>,
        <B_POS>, tau (polstat 3).  Written under `nomap` as well, as in the reference (:3655).  R[CELLS, columns of EMITTED]: the
        polarisation reduction factor per frequency from the emission stage, used where the ini has no `polred` -- every map with
        the column of its frequency (the reference needs that column copied into a `polred` file by hand, A2E_MABU.py:1190-1195)."""
        U, e = self.U, self.eng
        if not (U.POLMAP > 0 and U.NPIX[1] > 0):
            return []
        if len(getattr(U, "file_polred", "")) > 0:
            R = None
        I1, sel = self.polmap_frequencies()
        views, centre, KK, LENGTH_f, pix = self._view()
        polred = int(U.POLSTAT != 3 and (len(getattr(U, "file_polred", "")) > 0 or R is not None))    # -D POLRED (ASOC.py:349,359)
        p0 = float("%.4f" % U.p0)                                                               # -D p00=%.4ff
        written = []
        for IFREQ, EMIT, ABS, SCA in self._polmap_steps(EMITTED, R, I1, sel, KK, False):
            for idir, (d, ra, de) in enumerate(views):
                MAP = e.polmap(EMIT, d, ra, de, U.NPIX, U.MAP_DX, centre, ABS, SCA, polstat=int(U.POLSTAT),
                               polred=polred, rho_weight=int(U.POL_RHO_WEIGHT > 0), p0=p0, LENGTH=LENGTH_f)
                if self.rank != 0:
                    continue
                name = "polmap_%.1f_%02d.fits" % (1.0e4 * launch.C_LIGHT / float(self.FFREQ[IFREQ]), idir)          # f2um (:3800)
                files.write_fits(name, np.asarray(MAP, np.float32).reshape(4, U.NPIX[1], U.NPIX[0]), U.FITS_RA, U.FITS_DE, pix, planes=True)
                written.append(name)
        return written

    def write_healpix_polmaps(self, EMITTED, R=None):
        """`polmap bx by bz [[minlos] maxlos]` with `mapping NSIDE -1 dx` and `perspective x y z`: all-sky polarisation maps
        seen from inside the model (ASOC.py:3808-3958 -> PolHealpixMapping, kernel_ASOC_map_H.c, POLSTAT 0): for every
        frequency of the emitted range inside `wavelength` (:3911-3918; no `mapum` in this branch) pol_healpix.fits.<IFREQ>,
        a Healpix table with the columns I_STOKES, Q_STOKES, U_STOKES [Jy/sr] and N.  Unlike the flat maps these are not
        written under `nomap` (:3808).  `interpolate` and `yshear` act here, and only here.  R: as in write_polmaps.
        The field carries `polred` as THIS branch of the reference encodes it (:3867-3869): a file's R is not clipped and
        nothing is added under the root -- unlike the flat branch (:3710-3716)."""
        U, e = self.U, self.eng
        if not (U.POLMAP > 0 and U.NOMAP == 0 and U.NPIX[1] < 0):
            return []
        if len(getattr(U, "file_polred", "")) > 0:
            R = None
        polred = int(len(getattr(U, "file_polred", "")) > 0 or R is not None)                    # -D POLRED (ASOC.py:349,359)
        I1, sel = self._inside_wavelength()
        _, _, KK, LENGTH_f, _ = self._view()
        p0 = float("%.4f" % U.p0)                                                               # -D p00=%.4ff (ASOC.py:349)
        minlos, maxlos = float("%.3e" % U.MINLOS), float("%.3e" % U.MAXLOS)                      # -D MINLOS=%.3ef -D MAXLOS=%.3ef
        NSIDE = int(U.NPIX[0])
        written = []
        for IFREQ, EMIT, ABS, SCA in self._polmap_steps(EMITTED, R, I1, sel, KK, True):
            MAP = e.polmap_healpix(EMIT, NSIDE, U.INTOBS, ABS, SCA, polred=polred, p0=p0, interpolate=int(U.INTERPOLATE), minlos=minlos,
                                   maxlos=maxlos, y_shear=float(U.Y_SHEAR), LENGTH=LENGTH_f)
            if self.rank != 0:
                continue
            name = "pol_healpix.fits.%d" % IFREQ
            files.write_healpix_fits(name, np.asarray(MAP, np.float32).reshape(4, -1), files.HEALPIX_POL_COLUMNS, NSIDE)
            written.append(name)
        return written

    def write_ps_tau(self):
        """`pssavetau file um`: for every observer direction <file>_<idir>.dat with one line per point source -- its index,
        the column density [cm-2 per unit density] and the optical depth towards the observer at the frequency of the grid
        closest to `um` (ASOC.py:3576-3645, PSTau)"""
        U, e = self.U, self.eng
        IFREQ = int(np.argmin(np.abs(self.FFREQ - U.pssavetau_freq)))
        ABS, SCA = self._optical_for(IFREQ)
        views, _, _, LENGTH_f, _ = self._view()
        for idir, (d, _, _) in enumerate(views):
            col, tau = e.ps_tau(U.PSPOS[:U.NO_PS, :3], d, ABS, SCA, LENGTH_f)
            if self.rank == 0:
                with open("%s_%d.dat" % (U.file_pssavetau, idir), "w") as fp:
                    for i in range(U.NO_PS):
                        fp.write('%6d  %12.4e  %12.4e\n' % (i, col[i], tau[i]))
