#!/usr/bin/env python3
"""Generate tests/golden/zeeman_patterns.npz: the Zeeman patterns the UNMODIFIED reference computes for the lines of its five model
atoms (rh_atoms.py; atomic_model.py: VoigtLine.zeeman_components, effective_lande), and for the same lines with gLandeEff set to
two values.  The reference is imported the way make_golden.py imports it.  Numbers and names only are written:

  atoms                    names of the atoms, [5]
  line_atom, line_index    per recorded line: its atom (index into atoms) and its place among the atom's lines
  lower, upper             per line [3] each: J, L, S of its levels as float64; NaN where the level does not carry them
  ls                       per line: 1 where both levels are LS coupled for the reference
  gset                     per line: NaN (gLandeEff left None) or the value gLandeEff was set to
  has                      per line: 1 where zeeman_components() returned a pattern
  ptr                      [nlines + 1] into alpha / strength / shift
  alpha, strength, shift   the components of all patterns one after the other
  geff                     per line: effective_lande(), NaN where it raises for want of quantum numbers
One synthetic line without quantum numbers (a copy of a real line whose levels' J, L, S are set to None) closes the list.

Usage:  python tests/golden/make_zeeman_golden.py [--check]
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

GSETS = (1.1, 2.5)
ATOMS = ('H_6_atom', 'MgII_atom', 'CaII_atom', 'C_atom', 'Fe_simple_atom')


def _qn(level):
    return [np.nan if getattr(level, k) is None else float(getattr(level, k)) for k in ('J', 'L', 'S')]


def build():
    import make_golden as mg  # noqa: F401  (puts the reference and the stand-ins on sys.path)
    import rh_atoms
    import atomic_model as am
    rec = dict(line_atom=[], line_index=[], lower=[], upper=[], ls=[], gset=[], has=[], geff=[])
    ptr, alpha, strength, shift = [0], [], [], []

    def record(a, li, line):
        rec['line_atom'].append(a); rec['line_index'].append(li)
        rec['lower'].append(_qn(line.iLevel)); rec['upper'].append(_qn(line.jLevel))
        rec['ls'].append(int(bool(line.iLevel.lsCoupling and line.jLevel.lsCoupling)))
        rec['gset'].append(np.nan if line.gLandeEff is None else float(line.gLandeEff))
        z = line.zeeman_components()
        rec['has'].append(int(z is not None))
        if z is not None:
            alpha.extend(int(x) for x in z.alpha); strength.extend(float(x) for x in z.strength); shift.extend(float(x) for x in z.shift)
        ptr.append(len(alpha))
        try:
            rec['geff'].append(float(am.effective_lande(line)))
        except ValueError:
            rec['geff'].append(np.nan)

    last = None
    for a, name in enumerate(ATOMS):
        atom = getattr(rh_atoms, name)()
        for li, line in enumerate(atom.lines):
            for g in (None,) + GSETS:
                ln = copy.copy(line)
                ln.gLandeEff = g
                record(a, li, ln)
            last = (a, li, line)
    a, li, line = last
    bare = copy.copy(line)
    bare.gLandeEff = None
    bare.iLevel, bare.jLevel = copy.copy(line.iLevel), copy.copy(line.jLevel)
    for lev in (bare.iLevel, bare.jLevel):
        lev.J = lev.L = lev.S = None
        lev.lsCoupling = False
    record(a, -1, bare)
    out = dict(atoms=np.array([n[:-5] for n in ATOMS]), ptr=np.array(ptr, dtype=np.int64), alpha=np.array(alpha, dtype=np.int32),
               strength=np.array(strength, dtype=np.float64), shift=np.array(shift, dtype=np.float64))
    for k, v in rec.items():
        out[k] = np.array(v, dtype=np.float64 if k in ('lower', 'upper', 'gset', 'geff') else np.int32)
    return out


def main():
    path = os.path.join(HERE, 'zeeman_patterns.npz')
    d = build()
    if '--check' in sys.argv:
        old = np.load(path)
        assert sorted(old.files) == sorted(d), (sorted(old.files), sorted(d))
        for k in d:
            assert np.array_equal(old[k], d[k], equal_nan=d[k].dtype.kind == 'f'), k
        print('zeeman_patterns.npz is what the reference gives: %d lines, %d components' % (d['has'].shape[0], d['alpha'].shape[0]))
        return
    # np.savez writes member timestamps: write the members ourselves so that the file is byte-reproducible
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(d[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())
    print('wrote %s: %d lines, %d components, largest pattern %d, %d bytes'
          % (path, d['has'].shape[0], d['alpha'].shape[0], int(np.max(np.diff(d['ptr']))), os.path.getsize(path)))


if __name__ == '__main__':
    main()
