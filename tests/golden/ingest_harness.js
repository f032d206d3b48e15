'use strict';
/*
 * ingest_harness.js — TEST INFRASTRUCTURE.  Runs the UNMODIFIED reference bundle on oracle/canvas_shim.js (like oracle/ref_harness.js)
 * with a `video` LARGER than the work canvas, so that the loop's first line — canvasContext.drawImage(videoElement, 0, 0,
 * canvasElement.width, canvasElement.height), main.js:170 — scales, and records per frame the CRC-32 of the canvas after the draw and
 * the tracking object of the reference run on that canvas.
 *
 *   node tests/golden/ingest_harness.js job.json out.json       (driven by tests/golden/make_ingest_golden.py)
 *
 * job.json: { cases: [ {name, kind, vw, vh, w, h, frames: [raw RGBA files of vw x vh], params} ] }
 *   kind "facetrackr": the harness draws the video onto the canvas exactly as main.js:170 does, then facetrackr.Tracker.track()
 *   kind "mainjs":     the reference's own headtrackr.Tracker loop, init(video, canvas, false): ITS drawImage call scales
 */
const fs = require('fs');
const path = require('path');
const shim = require(path.join(__dirname, '..', '..', 'oracle', 'canvas_shim.js'));

const refPath = process.env.HT_REFERENCE_JS || '/root/reference/headtrackr.js';
global.document = shim.makeDocument();
global.window = global;
const headtrackr = require(refPath);

const CRC_TABLE = (function () {
  const t = new Int32Array(256);
  for (let n = 0; n < 256; n++) {
    let c = n;
    for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1);
    t[n] = c;
  }
  return t;
})();
function crc32All(buf) {
  let c = -1;
  for (let i = 0; i < buf.length; i++) c = CRC_TABLE[(c ^ buf[i]) & 0xFF] ^ (c >>> 8);
  return (c ^ -1) >>> 0;
}

function runFacetrackr(cs, base) {
  const out = { name: cs.name, kind: cs.kind, vw: cs.vw, vh: cs.vh, w: cs.w, h: cs.h, params: cs.params, calls: [] };
  const video = new shim.Canvas(cs.vw, cs.vh), canvas = new shim.Canvas(cs.w, cs.h);
  const ft = new headtrackr.facetrackr.Tracker(Object.assign({}, cs.params));
  ft.init(canvas);
  for (let i = 0; i < cs.frames.length; i++) {
    video.loadRGBA(fs.readFileSync(path.resolve(base, cs.frames[i])));
    canvas.getContext('2d').drawImage(video, 0, 0, canvas.width, canvas.height);   /* main.js:170 */
    const crc = crc32All(canvas._buf);
    ft.track();
    const t = ft.getTrackingObject();
    out.calls.push({ frame: i, canvas_crc: crc, x: t.x, y: t.y, width: t.width, height: t.height, angle: t.angle, confidence: t.confidence, detection: t.detection });
  }
  return out;
}

function runMainJs(cs, base) {
  const out = { name: cs.name, kind: cs.kind, vw: cs.vw, vh: cs.vh, w: cs.w, h: cs.h, params: cs.params, calls: [] };
  const video = new shim.Canvas(cs.vw, cs.vh), canvas = new shim.Canvas(cs.w, cs.h);
  video.currentTime = 1; video.paused = false; video.ended = false; video.addEventListener = function () {}; video.style = {};
  let parked = null;
  const realSetTimeout = global.setTimeout, realClear = global.clearTimeout;
  global.setTimeout = function (fn) { parked = fn; return 1; };   /* the loop's re-arm (main.js:302-304) is parked and fired per frame */
  global.clearTimeout = function () { parked = null; };
  const status = [], faces = [];
  const sl = function (e) { status.push(e.status); };
  const fl = function (e) { faces.push({ x: e.x, y: e.y, width: e.width, height: e.height, angle: e.angle, confidence: e.confidence, detection: e.detection }); };
  document.addEventListener('headtrackrStatus', sl);
  document.addEventListener('facetrackingEvent', fl);
  try {
    const tr = new headtrackr.Tracker(Object.assign({ ui: false, debug: false }, cs.params));
    tr.init(video, canvas, false);
    for (let i = 0; i < cs.frames.length; i++) {
      status.length = 0; faces.length = 0;
      video.loadRGBA(fs.readFileSync(path.resolve(base, cs.frames[i])));
      if (i === 0) tr.start(); else { const fn = parked; parked = null; if (fn) fn(); }
      /* nothing after main.js:170 writes the work canvas, so its pixels after the step are the pixels after the draw */
      const call = { frame: i, canvas_crc: crc32All(canvas._buf), status: status.slice() };
      if (faces.length) Object.assign(call, faces[faces.length - 1]);                 /* facetrackr.js:112-125: CS frames only */
      else call.detection = status.indexOf('whitebalance') >= 0 ? 'WB' : status.indexOf('detecting') >= 0 ? 'VJ' : null;
      out.calls.push(call);
    }
    tr.stop();
  } finally {
    global.setTimeout = realSetTimeout; global.clearTimeout = realClear;
    document.removeEventListener('headtrackrStatus', sl);
    document.removeEventListener('facetrackingEvent', fl);
  }
  return out;
}

function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
  const base = path.dirname(path.resolve(process.argv[2]));
  const res = { reference_rev: headtrackr.rev, node: process.version, cases: [] };
  job.cases.forEach(function (cs) {
    const r = cs.kind === 'mainjs' ? runMainJs(cs, base) : runFacetrackr(cs, base);
    r.gen = cs.gen;
    res.cases.push(r);
  });
  fs.writeFileSync(process.argv[3], JSON.stringify(res));
}
main();
