"""Extracts the light and camera VALUES of the one scene file the reference ships
(CommonPasses/Data/pink_room/pink_room.fscene) into tests/golden/pink_room_values.json.

Usage: python tests/golden/make_pink_room_fixture.py <pink_room.fscene of a reference checkout>
Only numbers and names are kept (lights, cameras, active camera); the model entry is dropped because the
geometry blob it names is absent from the reference tree.
"""
import json
import os
import sys

DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pink_room_values.json")

if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        scene = json.load(f)
    out = {"source": "CommonPasses/Data/pink_room/pink_room.fscene", "version": scene.get("version"),
           "active_camera": scene.get("active_camera"), "lights": scene.get("lights", []), "cameras": scene.get("cameras", [])}
    with open(DST, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", DST, len(out["lights"]), "lights", len(out["cameras"]), "cameras")
