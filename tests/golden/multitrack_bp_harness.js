'use strict';
/*
 * multitrack_bp_harness.js — TEST INFRASTRUCTURE.  Runs the UNMODIFIED reference bundle on oracle/canvas_shim.js (like
 * tests/golden/multitrack_harness.js) with SEVERAL camshift.Tracker instances on one canvas and records, per tracker and track() call,
 * the debug surface of the reference: the CRC-32 of getBackProjectionImg().data (camshift.js:177-196) and a handful of getPdf()
 * samples (camshift.js:172-175), as [x, y, value].
 *
 *   HT_REFERENCE_JS=<reference headtrackr.js> node tests/golden/multitrack_bp_harness.js job.json out.json
 *   (driven by tests/golden/make_multitrack_bp_golden.py)
 *
 * job.json: { cases: [ {name, w, h, rects: [[x, y, w, h], ...], frames: [raw RGBA files of w x h], samples: [[x, y], ...]} ] }
 */
const fs = require('fs');
const path = require('path');
const zlib = require('zlib');
const shim = require(path.join(__dirname, '..', '..', 'oracle', 'canvas_shim.js'));

const refPath = process.env.HT_REFERENCE_JS; /* the reference bundle headtrackr.js, outside this repository */
if (!refPath) { console.error('multitrack_bp_harness.js: set HT_REFERENCE_JS to the reference headtrackr.js'); process.exit(2); }
global.document = shim.makeDocument();
global.window = global;
const headtrackr = require(refPath);

let table = null;
function crc32(buf) {
  if (typeof zlib.crc32 === 'function') return zlib.crc32(buf) >>> 0;
  if (!table) {
    table = new Uint32Array(256);
    for (let n = 0; n < 256; n++) {
      let c = n;
      for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1);
      table[n] = c >>> 0;
    }
  }
  let c = 0xFFFFFFFF;
  for (let i = 0; i < buf.length; i++) c = table[(c ^ buf[i]) & 0xFF] ^ (c >>> 8);
  return (c ^ 0xFFFFFFFF) >>> 0;
}

function run(cs, base) {
  const out = { name: cs.name, w: cs.w, h: cs.h, rects: cs.rects, trackers: [] };
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
      const img = t.getBackProjectionImg(), pdf = t.getPdf();
      out.trackers[j].push({
        frame: i,
        crc: crc32(Buffer.from(img.data.buffer, img.data.byteOffset, img.data.length)),
        pdf: cs.samples.map(function (p) { return [p[0], p[1], pdf[p[0]][p[1]]]; }),
      });
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
