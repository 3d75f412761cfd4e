"""Records tests/golden/xbot_l_leg_joints.json from the robot description: for both legs, every joint on the chain from `base_link`
down to the ankle-roll link -- name, type, parent and child link, origin xyz / rpy, axis and limits -- in chain order.  Data only;
tests/test_symmetry.py runs zero-pose forward kinematics on it to check the mirror signs of the joint table.

    python tests/golden/gen_leg_joints_fixture.py <path to XBot-L.urdf>
"""
import json
import os
import sys
import xml.etree.ElementTree as ET

HERE = os.path.dirname(os.path.abspath(__file__))
LEG_JOINTS = ("leg_roll", "leg_yaw", "leg_pitch", "knee", "ankle_pitch", "ankle_roll")      # the DOF order within one leg


def floats(text, default):
    return [float(x) for x in text.split()] if text else list(default)


def main(urdf):
    root = ET.parse(urdf).getroot()
    by_child = {}
    for j in root.findall("joint"):
        origin, axis, limit = j.find("origin"), j.find("axis"), j.find("limit")
        by_child[j.find("child").get("link")] = dict(
            name=j.get("name"), type=j.get("type"), parent=j.find("parent").get("link"), child=j.find("child").get("link"),
            xyz=floats(origin.get("xyz") if origin is not None else None, (0.0, 0.0, 0.0)),
            rpy=floats(origin.get("rpy") if origin is not None else None, (0.0, 0.0, 0.0)),
            axis=floats(axis.get("xyz") if axis is not None else None, (1.0, 0.0, 0.0)),
            lower=float(limit.get("lower")) if limit is not None and limit.get("lower") is not None else None,
            upper=float(limit.get("upper")) if limit is not None and limit.get("upper") is not None else None)
    out = dict(base="base_link", dof_order=["%s_%s_joint" % (side, n) for side in ("left", "right") for n in LEG_JOINTS], chains={})
    for side in ("left", "right"):
        last = next(j for j in by_child.values() if j["name"] == "%s_ankle_roll_joint" % side)
        chain, link = [], last["child"]
        while link != out["base"]:
            chain.append(by_child[link])
            link = by_child[link]["parent"]
        out["chains"][side] = chain[::-1]
    path = os.path.join(HERE, "xbot_l_leg_joints.json")
    json.dump(out, open(path, "w"), indent=1)
    print(path, {k: [j["name"] for j in v] for k, v in out["chains"].items()})


if __name__ == "__main__":
    main(sys.argv[1])
