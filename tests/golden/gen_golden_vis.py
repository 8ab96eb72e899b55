#!/usr/bin/env python
"""Part labels and link name pairs of the REAL reference's utils/vis.py, as data.

Run in the build container only (needs the reference checkout):

    python tests/golden/gen_golden_vis.py

The reference module imports cv2 and cannot be imported here, so its source is parsed with ``ast`` and the four
literal tables (coco_part_labels, coco_part_orders, crowd_pose_part_labels, crowd_pose_part_orders) are evaluated with
``ast.literal_eval``; none of its text is kept.  nano_demo/utils/vis.py and lib/dataset/__init__.py (where lib/utils/vis.py
takes its VIS_CONFIG from) must agree.  Stored in
tests/golden/vis_tables.json: {'COCO' | 'CROWDPOSE': {'part_labels': [name], 'part_orders': [[name, name]]}} -- lists
of names and name pairs only.  tests/test_vis_cpu.py holds litepose_amd.utils.vis.VIS_CONFIG to it.
"""
import ast
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get('LITEPOSE_REFERENCE', '/root/reference')
NAMES = {'COCO': ('coco_part_labels', 'coco_part_orders'),
         'CROWDPOSE': ('crowd_pose_part_labels', 'crowd_pose_part_orders')}


def tables(path):
    with open(path) as f:
        tree = ast.parse(f.read())
    found = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            name = node.targets[0].id
            if any(name in pair for pair in NAMES.values()):
                found[name] = ast.literal_eval(node.value)
    return {ds: {'part_labels': list(found[lab]), 'part_orders': [list(p) for p in found[orders]]}
            for ds, (lab, orders) in NAMES.items()}


def main():
    a = tables(os.path.join(REFERENCE, 'nano_demo', 'utils', 'vis.py'))
    b = tables(os.path.join(REFERENCE, 'lib', 'dataset', '__init__.py'))
    assert a == b, 'nano_demo/utils/vis.py and lib/dataset/__init__.py disagree'
    assert len(a['COCO']['part_orders']) == 19 and len(a['CROWDPOSE']['part_orders']) == 15
    out = os.path.join(HERE, 'vis_tables.json')
    with open(out, 'w') as f:
        json.dump(a, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
