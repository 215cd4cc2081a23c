"""Depth maps of a database's views by plane-sweep stereo (neuray_amd/stereo.py).

    python -m neuray_amd.estimate_depth --database NAME [--planes D --radius R --src S --max-cost C --no-geometric] [--write [--root DIR]] [--overwrite]

prints the coverage of every view (the share of its pixels - of its mask where the database has one - that get a depth) and, on a procedural
database, the error against the true depth; one JSON line at the end.  --write stores each map with write_colmap_array where the database's
get_depth looks for it (<root>/colmap_depth/<id>.jpg.geometric.bin; --root: another directory, needed for a database that keeps no files)
and refuses to replace an existing file without --overwrite."""
import argparse
import json
import os

import numpy as np

from . import database as _database
from . import procedural, stereo


def run(args):
    db = _database.parse_database_name(args.database)
    ids = list(db.get_img_ids())
    paths = None
    if args.write:
        try:
            paths = [stereo.depth_path(db, i, args.root) for i in ids]
        except ValueError as e:
            raise SystemExit(str(e) + " (--root)")
        there = [p for p in paths if os.path.exists(p)]
        if there and not args.overwrite:      # before any work and before any file is written
            raise SystemExit("neuray_amd.estimate_depth: %s exists (%d of %d files): --overwrite replaces them" % (there[0], len(there), len(paths)))
    maps = stereo.stereo_depth_maps(db, ids, src=args.src, planes=args.planes, radius=args.radius, max_cost=args.max_cost,
                                    geometric=not args.no_geometric)
    depth = maps['depth']
    synthetic_truth = isinstance(db, procedural.ProceduralDatabase)
    views = []
    for k, i in enumerate(ids):
        mask = np.asarray(db.get_mask(i)) > 0
        got = (depth[k] > 0) & mask
        row = {'id': i, 'coverage': float(got.sum() / max(mask.sum(), 1))}
        if synthetic_truth:
            true = np.asarray(db.get_depth(i), np.float32)
            sel = got & (true > 0)
            rel = np.abs(depth[k][sel] - true[sel]) / true[sel]
            row['median_rel_error'] = float(np.median(rel)) if rel.size else None
            row['outside_surface'] = float(((depth[k] > 0) & ~(true > 0)).sum() / max((depth[k] > 0).sum(), 1))
        print('view %s: coverage %.1f %%' % (i, 100 * row['coverage']) +
              (', median relative error %.2f %%' % (100 * row['median_rel_error']) if row.get('median_rel_error') is not None else ''))
        views.append(row)
    if paths:
        for k, p in enumerate(paths):
            _database.write_colmap_array(p, depth[k])
    errs = [v['median_rel_error'] for v in views if v.get('median_rel_error') is not None]
    res = {'database': args.database, 'views': len(ids), 'h': int(depth.shape[1]), 'w': int(depth.shape[2]),
           'coverage': float(np.mean([v['coverage'] for v in views])), 'median_rel_error': float(np.median(errs)) if errs else None,
           'written': paths or [], 'on': 'hip' if procedural._device_engine() is not None else 'numpy',
           'settings': {'src': args.src, 'planes': args.planes, 'radius': args.radius, 'max_cost': args.max_cost, 'geometric': not args.no_geometric},
           'per_view': views}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m neuray_amd.estimate_depth')
    ap.add_argument('--database', type=str, default=None, help="e.g. llff_colmap/fern_high or procedural/0/white_800")
    ap.add_argument('--planes', type=int, default=stereo.DEFAULTS['planes'])
    ap.add_argument('--radius', type=int, default=stereo.DEFAULTS['radius'])
    ap.add_argument('--src', type=int, default=stereo.DEFAULTS['src'])
    ap.add_argument('--max-cost', type=float, default=stereo.DEFAULTS['max_cost'])
    ap.add_argument('--no-geometric', action='store_true', help='keep the photometric depth, without geometry.filter_depth')
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--root', type=str, default=None, help='write under this directory instead of the database\'s own')
    ap.add_argument('--overwrite', action='store_true')
    args = ap.parse_args(argv)
    if not args.database:
        ap.error("--database is required")
    try:
        res = run(args)
    except ValueError as e:
        raise SystemExit(str(e))
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
