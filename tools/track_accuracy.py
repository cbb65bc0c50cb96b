"""The accuracy table of profiles/notes_track.md: the NumPy restatement of "Tracking" (tests/track_reference.py, no GPU) on
the 384 x 512 table scene, one object at a time -- the 7 cm cube, the L prism lying flat, the standing plate -- under the slow
(1.1 cm, 2 degrees per frame) and the fast motion (2.2 cm, 5 degrees per frame, from rest) of tests/test_track_host.py, from
a constant and a constant-velocity start, on clean frames and on frames that went through the 'kinect1' sensor model
(tests/depth_noise_reference.py).  Prints max |T - T_true| over the 4 x 4 entries per frame, and whether the track was lost.

    python tools/track_accuracy.py [--contour]

--contour adds the occluding-contour term of DESIGN.md "Contours" at its defaults (tests/contour_reference.py): the table of
profiles/notes_track_contour.md.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contour_reference as CR
import depth_noise_reference as DN
import detect_reference as DR
import render_reference as R
import track_reference as TR

PLACE = {0: ("prism", -0.24, 0.02, 0.02, [0.0, 0.0, 0.4]), 1: ("plate", 0.0, 0.05, 0.06, [np.pi / 2, 0.0, 0.0]),
         2: ("cube", 0.23, -0.02, 0.035, [0.0, 0.0, 0.7])}
DIRECTION = {0: 0.0, 1: 0.0, 2: None}              # the prism and the plate slide along the table's x; the cube as in the tests


def pose(obj, f, motion):
    if obj == 2:
        return TR.cube_pose(f, motion)
    step, degrees, _, _, from_rest = motion
    _, x, y, h, rot = PLACE[obj]
    s = max(f - 0.5, 0.0) if from_rest else float(f)
    turn = R.pose_matrix([0.0, 0.0, np.radians(degrees) * s], [0.0, 0.0, 0.0])
    return TR.TABLE_POSE @ R.pose_matrix([0.0, 0.0, 0.0], [x + step * s, y, h]) @ turn @ R.pose_matrix(rot, [0.0, 0.0, 0.0])


def main():
    parser = argparse.ArgumentParser(description="the restatement's tracking accuracy on the table scene")
    parser.add_argument("--contour", action="store_true", help="with the occluding-contour term at its defaults")
    run = CR.track if parser.parse_args().contour else TR.track
    meshes = DR.scene_meshes()
    intr = np.tile(TR.SCENE_INTR, (TR.FRAMES, 1))
    print("| object | motion | start | sensor | max abs T - T_true per frame | lost |")
    print("|---|---|---|---|---|---|")
    for obj in (2, 0, 1):
        for mname, motion in (("slow", TR.SLOW), ("fast", TR.FAST)):
            truth = np.array([pose(obj, f, motion) for f in range(TR.FRAMES)])
            fr = [[(TR.TABLE, 1, TR.TABLE_POSE), (obj, 2, truth[f])] for f in range(TR.FRAMES)]
            clean = R.render(meshes, fr, intr, TR.SCENE_H, TR.SCENE_W)
            noisy = DN.apply(clean['depth'], clean['label'], intr, DN.KINECT1,
                             seed=7, first_frame=0)
            for sname, depth in (("clean", clean['depth']), ("kinect1", noisy['depth'])):
                for start in ("constant", "velocity"):
                    r = run(depth, TR.SCENE_INTR, meshes, [obj], truth[:1], motion=start)
                    err = ["%.1e" % TR.pose_error(r['poses'][f, 0], truth[f]) for f in range(TR.FRAMES)]
                    print("| %s | %s | %s | %s | %s | %s |" % (PLACE[obj][0], mname, start, sname, " ".join(err),
                                                             "".join("x" if v else "." for v in r['lost'][:, 0])), flush=True)


if __name__ == "__main__":
    main()
