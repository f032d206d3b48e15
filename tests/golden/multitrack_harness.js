'use strict';
/*
 * multitrack_harness.js — TEST INFRASTRUCTURE.  Runs the UNMODIFIED reference bundle on oracle/canvas_shim.js (like oracle/ref_harness.js)
 * with SEVERAL camshift.Tracker instances on one canvas: frame 0 initialises tracker j on rects[j] (camshift.js:198-211), every later
 * frame is one track(canvas) of every tracker (camshift.js:213-353); per call the track object and the search window are recorded.
 *
 *   node tests/golden/multitrack_harness.js job.json out.json       (driven by tests/golden/make_multitrack_golden.py)
 *
 * job.json: { cases: [ {name, w, h, rects: [[x, y, w, h], ...], frames: [raw RGBA files of w x h], gen} ] }
 */
const fs = require('fs');
const path = require('path');
const shim = require(path.join(__dirname, '..', '..', 'oracle', 'canvas_shim.js'));

const refPath = process.env.HT_REFERENCE_JS || '/root/reference/headtrackr.js';
global.document = shim.makeDocument();
global.window = global;
const headtrackr = require(refPath);

function run(cs, base) {
  const out = { name: cs.name, w: cs.w, h: cs.h, rects: cs.rects, gen: cs.gen, trackers: [] };
  const canvas = new shim.Canvas(cs.w, cs.h);
  const trackers = cs.rects.map(function () { return new headtrackr.camshift.Tracker({ calcAngles: true }); });
  canvas.loadRGBA(fs.readFileSync(path.resolve(base, cs.frames[0])));
  trackers.forEach(function (t, j) {
    const r = cs.rects[j];
    t.initTracker(canvas, new headtrackr.camshift.Rectangle(r[0], r[1], r[2], r[3]));
    out.trackers.push([]);
  });
  for (let i = 1; i < cs.frames.length; i++) {
    canvas.loadRGBA(fs.readFileSync(path.resolve(base, cs.frames[i])));
    trackers.forEach(function (t, j) {
      t.track(canvas);
      const o = t.getTrackObj(), sw = t.getSearchWindow();
      out.trackers[j].push({ x: o.x, y: o.y, width: o.width, height: o.height, angle: o.angle, sw: [sw.x, sw.y, sw.width, sw.height] });
    });
  }
  return out;
}

function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
  const base = path.dirname(path.resolve(process.argv[2]));
  const res = { reference_rev: headtrackr.rev, node: process.version, cases: job.cases.map(function (cs) { return run(cs, base); }) };
  fs.writeFileSync(process.argv[3], JSON.stringify(res));
}
main();
